"""CPU suite: the features with a sticky setter of their own -- tiles, slices, fast decisions, motion search, LCU-level rate control -- in
combination.  The fixtures (tests/gen_golden_combo.py: clips the real reference encoded with two or three of them at once) are what they claim,
and the kernel source reproduces the six clips without rate control on the host twins, which take every switch: hostsim_tiles / hostsim_slices with
fast= and me=, hostsim_fast with me=.  A mismatch here is the fixture's or the shared kernel source's; one that shows on the GPU only is the
launch's (teams, ticket loops, the waits between chains).

Every clip is replayed whole: the I picture and its three P / B slices.  Measured, forwards plus reversed on one core: the full-search clips
combo_tiles_me_ra (+-16, 27 CTUs) 11.7 s, combo_tiles_fast_me_ldb (+-8, 26 CTUs) 3.5 s, combo_fast_me_rawpp (+-8, 9 CTUs; hostsim_fast skips
the I picture) 3.2 s; the others combo_tiles_fast_ldp 3.7 s, combo_slices_fast_ldb 4.9 s, combo_slices_me_ldp 4.9 s; building the six twin
binaries once per module 41 s.  So no clip needs the max_inter_slices cap, which a test of its own exercises."""
import os
import subprocess

import numpy as np
import pytest

import common
from slices_common import MAX_BYTES, fixed_ctu_slices, load_slices_case

COMBO_CASES = ["combo_tiles_fast_ldp", "combo_tiles_me_ra", "combo_tiles_fast_me_ldb", "combo_slices_fast_ldb", "combo_slices_me_ldp", "combo_fast_me_rawpp"]
RC_CASE = "combo_rc2_fast_me_ldpwpp"
ME_DEFAULTS = (1, 64, 4)
# what the issue fixes per clip: the features, the tile layout (columns, rows, uniform) or None, SliceArgument or 0, the switches, the search
COMBO_TABLE = {
    "combo_tiles_fast_ldp": (("tiles", "fast"), ((4, 5), (2, 1), 0), 0, (1, 1, 1), ME_DEFAULTS),
    "combo_tiles_me_ra": (("tiles", "me"), ((5, 4), (3,), 0), 0, (0, 0, 0), (0, 16, 2)),
    "combo_tiles_fast_me_ldb": (("tiles", "fast", "me"), ((4, 4, 5), (2,), 1), 0, (1, 0, 1), (0, 8, 4)),
    "combo_slices_fast_ldb": (("slices", "fast"), None, 7, (1, 1, 1), ME_DEFAULTS),
    "combo_slices_me_ldp": (("slices", "me"), None, 4, (0, 0, 0), (1, 24, 4)),
    "combo_fast_me_rawpp": (("fast", "me"), None, 0, (1, 1, 1), (0, 8, 2)),
    RC_CASE: (("fast", "me", "rc"), None, 0, (1, 1, 1), (1, 24, 4)),
}
# the first CTUs of the chains that start from the carried m_integerMv2Nx2N: the two bottom tiles; the slice that starts in the bottom CTU row
CARRY = {"combo_tiles_fast_ldp": [18, 22], "combo_slices_fast_ldb": [14]}


def combo_settings(name):
    """the settings of every feature as the fixture names them (the defaults for a feature the clip does not use)"""
    g = np.load(os.path.join(common.GOLD, name + ".npz"))
    return dict(features=tuple(str(f) for f in g["features"]), cols=tuple(int(v) for v in g["tile_cols"]), rows=tuple(int(v) for v in g["tile_rows"]),
                uniform=int(g["tile_uniform"]), first=[int(v) for v in g["slice_first_ctu"]], slice_arg=int(g["slice_arg"]),
                fast=tuple(int(g[k]) for k in ("esd", "cfm", "ecu")), me=tuple(int(g[k]) for k in ("fast_search", "search_range", "bipred_search_range")),
                qp=int(g["qp"]), diff={f: g[f"diff_ctus_without_{f}"] for f in g["features"]})


def test_combo_fixtures_cover_what_they_are_for():
    """every clip: the features, layout and switches the table above fixes; partial CTUs at the bottom (and on the right where there is a
    layout); three inter pictures or more; every feature matters -- without tiles / slices alone at least half of the CTUs of every picture
    differ, without the fast decisions / the motion search alone two inter pictures or more differ, and the rate model moved the QP of a CTU;
    the first CTU of a bottom tile / a later slice the picture edge cuts differs from the run without the fast decisions; below 700,000 bytes"""
    assert sorted(COMBO_TABLE) == sorted(COMBO_CASES + [RC_CASE])
    for name, (features, tiles, arg, fast, me) in COMBO_TABLE.items():
        g = np.load(os.path.join(common.GOLD, name + ".npz"))
        cfg, slices, finals, sao, bits, extra = load_slices_case(name)
        s = combo_settings(name)
        w_ctu, h_ctu = (cfg["width"] + 63) // 64, (cfg["height"] + 63) // 64
        n = w_ctu * h_ctu
        assert cfg["height"] % 64 and (cfg["width"] % 64 or not (tiles or arg)), name
        assert s["features"] == features and s["fast"] == fast and s["me"] == me and len(features) >= 2, name
        assert (s["cols"], s["rows"], s["uniform"]) == (tiles or ((w_ctu,), (h_ctu,), 0)), name
        assert s["slice_arg"] == arg and s["first"] == (fixed_ctu_slices(w_ctu, h_ctu, cfg["wpp"], arg) if arg else [0]), name
        assert cfg["wpp"] == (0 if tiles or arg else 1), name
        assert ("fast" in features) == (sum(fast) > 0) and ("me" in features) == (me != ME_DEFAULTS), name
        assert len(slices) == cfg["frames"] == len(finals) == len(sao) == len(bits) and len(set(int(r["poc"]) for r in slices)) == len(slices), name
        inter = [k for k, r in enumerate(slices) if int(r["slice_type"]) != 2]
        assert len(inter) >= 3, name
        for r in slices:                                               # one substream per tile / per CTU row, one 'B' record per slice
            b = bits[int(r["poc"])]
            assert len(b) == len(s["first"]), name
            if arg:
                assert all(sum(len(x) > 0 for x in rec["substreams"]) == 1 for rec in b), name
            else:
                assert len(b[0]["substreams"]) == (h_ctu if cfg["wpp"] else len(s["cols"]) * len(s["rows"])), name
        for f in features:
            d = s["diff"][f]
            assert len(d) == len(slices), name
            if f in ("tiles", "slices"):
                assert all(2 * int(v) >= n for v in d), f"{name} without {f}: {d}"
            elif f in ("fast", "me"):
                assert sum(int(d[k]) > 0 for k in inter) >= 2, f"{name} without {f}: {d}"
        if "rc" in features:
            assert all(r["lcu_rc"] is not None and r["dqp"] is not None for r in slices), name
            assert any((np.asarray(r["lcu_rc"]["ctu_qp"]) != int(r["qp"])).any() for r in slices if int(r["slice_type"]) != 2), name
        else:
            assert all(r["lcu_rc"] is None and r["dqp"] is None for r in slices), name
        if name in CARRY:
            assert [int(v) for v in g["carry_first_ctus"]] == CARRY[name], name
            for a in CARRY[name]:                                      # first of its chain, not of the picture, cut by the picture edge
                assert a and ((a % w_ctu) * 64 + 63 >= cfg["width"] or (a // w_ctu) * 64 + 63 >= cfg["height"]), name
            dc = g["diff_carry_ctus_without_fast"]
            assert dc.shape == (len(slices), len(CARRY[name])) and dc[inter].any(), f"{name}: {dc}"
        else:
            assert "carry_first_ctus" not in g, name
        assert os.path.getsize(os.path.join(common.GOLD, name + ".npz")) < MAX_BYTES, name


# ---- the host twins ----
def _csv(v):
    return ",".join(str(int(x)) for x in v)


def twin_command(name, tmp_path, twins, which="fwd", without=None):
    """the twin that matches the clip's layout and its arguments, the feature `without` left off -> (argument list, inter slices in the clip)"""
    import hmd2
    import synth
    recs = []
    cfg, slices, _ = common.load_ldp_case(name, recs)
    s = combo_settings(name)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump2.bin"
    if not yuv.exists():
        synth.write_yuv(str(yuv), w, h, bd, cfg["frames"], cfg["seed"])
        hmd2.write(str(dump), recs)
    fast = "fast=%d%d%d" % (s["fast"] if without != "fast" else (0, 0, 0))
    me = "me=%d,%d,%d" % (s["me"] if without != "me" else ME_DEFAULTS)
    head = [str(yuv), str(dump), str(w), str(h), str(bd)]
    if "tiles" in s["features"]:
        args = [str(twins["tiles"][which])] + head + (["0", "0"] if without == "tiles" else [_csv(s["cols"]), _csv(s["rows"])]) + [me, fast]
    elif "slices" in s["features"]:
        args = [str(twins["slices"][which])] + head + ["0" if without == "slices" else _csv(s["first"])] + [fast, me]
    else:
        args = [str(twins["fast"][which])] + head + [str(cfg["wpp"])] + [fast[5], fast[6], fast[7], me]
    return args, sum(int(r["slice_type"]) != 2 for r in slices)


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostsim_combo")
    return {k: {"fwd": common.build_hostsim(d, "hostsim_" + k), "rev": common.build_hostsim(d, "hostsim_" + k, "-DHM355_HOSTSIM_REVERSE", exe=f"hostsim_{k}_rev")}
            for k in ("tiles", "slices", "fast")}


@pytest.mark.parametrize("name", COMBO_CASES)
def test_hostsim_matches_reference_with_the_combined_settings(tmp_path, twins, name):
    """the kernel source on the host with one lane, forwards and with every lane-parallel loop reversed, with every setting the fixture names:
    every slice bit for bit (decisions, motion, coefficients, costs, reconstruction)"""
    for which in ("fwd", "rev"):
        args, n_inter = twin_command(name, tmp_path, twins, which)
        r = subprocess.run(args, capture_output=True, text=True)
        assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
        assert r.stdout.count(": ok\n") == n_inter + ("fast" not in os.path.basename(args[0])), r.stdout[-2000:]      # (hostsim_fast skips the I picture)


@pytest.mark.parametrize("name,without", [(n, f) for n in COMBO_CASES for f in COMBO_TABLE[n][0]])
def test_hostsim_with_one_feature_off_does_not_reproduce_the_clip(tmp_path, twins, name, without):
    """each feature of each clip matters to the twin as it did to the reference: left off alone, the replay ends in a mismatch"""
    args, _ = twin_command(name, tmp_path, twins, "fwd", without)
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 1 and "MISMATCH" in r.stdout, f"{name} should not be reproduced without {without}: " + r.stdout[-1000:] + r.stderr[-500:]


def test_twins_refuse_malformed_switches(tmp_path, twins):
    args, _ = twin_command(COMBO_CASES[0], tmp_path, twins)
    for bad in ("fast=12", "me=0,8", "tiles=2x2"):
        r = subprocess.run(args + [bad], capture_output=True, text=True)
        assert r.returncode == 2, bad


def test_max_inter_slices_ends_the_replay_early(tmp_path, twins):
    """hostsim_me's cap in the three twins that now take me=: the I picture and one inter slice, and still "all bit-exact" """
    for name in ("combo_tiles_fast_me_ldb", "combo_slices_me_ldp", "combo_fast_me_rawpp"):
        d = tmp_path / name
        d.mkdir()
        args, _ = twin_command(name, d, twins)
        r = subprocess.run(args + ["max_inter_slices=1"], capture_output=True, text=True)
        assert r.returncode == 0 and "all bit-exact" in r.stdout and r.stdout.count(": ok\n") == 1 + ("fast" not in os.path.basename(args[0])), r.stdout[-1000:]
