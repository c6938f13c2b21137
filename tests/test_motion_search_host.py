"""CPU suite: the motion search of hm355_set_motion_search (the reference's --FastSearch / --SearchRange / --BipredSearchRange) in the kernel
source, on the host twin tests/hostsim/hostsim_me.cpp against clips the real reference encoded with those options (tests/gen_golden_me.py)."""
import os
import subprocess

import numpy as np
import pytest

import common

ME_FULL_CASES = ["me_full8_ldp_192x128_8b_qp32", "me_full16_ldpwpp_200x136_8b_qp30", "me_full8_ra_192x128_10b_qp32", "me_full32_ldp_136x72_8b_qp28"]
ME_CASES = ME_FULL_CASES + ["me_tz24_ldp_200x136_8b_qp30", "me_tz128_bi8_ldb_136x72_8b_qp30"]
ME_DEFAULTS = (1, 64, 4)
# the twin's legs: clip -> inter slices replayed (None: all of them)
HOST_CASES = {"me_full8_ldp_192x128_8b_qp32": None, "me_full16_ldpwpp_200x136_8b_qp30": None, "me_tz24_ldp_200x136_8b_qp30": None,
              "me_tz128_bi8_ldb_136x72_8b_qp30": None}


def me_settings(name):
    g = np.load(os.path.join(common.GOLD, name + ".npz"))
    return tuple(int(g[k]) for k in ("fast_search", "search_range", "bipred_search_range"))


def _replay_inputs(tmp_path, name):
    """the clip and the HMD2 stream of its 'S' / 'F' records for hostsim_me -> argument list"""
    import hmd2
    import synth
    recs = []
    cfg, slices, _ = common.load_ldp_case(name, recs)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump2.bin"
    synth.write_yuv(str(yuv), w, h, bd, cfg["frames"], cfg["seed"])
    hmd2.write(str(dump), recs)
    return cfg, [str(yuv), str(dump), str(w), str(h), str(bd), str(cfg["wpp"])]


def test_fixtures_differ_from_the_reference_with_the_default_search():
    """every clip names its settings and has three inter slices or more; the reference's own decisions change against its run with 1 / 64 / 4 in
    two inter pictures or more of every full-search clip and in one or more of the TZ clip with range 24 (me_tz128_bi8 carries no condition)"""
    need = {name: 2 for name in ME_FULL_CASES}
    need["me_tz24_ldp_200x136_8b_qp30"] = 1
    need["me_tz128_bi8_ldb_136x72_8b_qp30"] = 0
    for name in ME_CASES:
        g = np.load(os.path.join(common.GOLD, name + ".npz"))
        _, slices, _ = common.load_ldp_case(name)
        diff = g["diff_ctus_vs_off"]
        fs, sr, bi = me_settings(name)
        assert len(diff) == len(slices) and (fs, sr, bi) != ME_DEFAULTS and fs in (0, 1) and 1 <= sr <= 256 and 1 <= bi <= 16
        assert fs == (0 if name in ME_FULL_CASES else 1)
        inter = [int(d) for r, d in zip(slices, diff) if int(r["slice_type"]) != 2]
        assert len(inter) >= 3 and sum(d > 0 for d in inter) >= need[name], f"{name}: {inter}"
        assert os.path.getsize(os.path.join(common.GOLD, name + ".npz")) < 700000


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_hostsim_me_matches_reference_with_the_settings(tmp_path, name):
    """the kernel source on the host with one lane, forwards and with every lane-parallel loop reversed, with the settings the fixture names:
    every P / B slice bit for bit (decisions, motion, coefficients, costs, reconstruction)"""
    cfg, args = _replay_inputs(tmp_path, name)
    settings = [str(v) for v in me_settings(name)]
    tail = [str(HOST_CASES[name])] if HOST_CASES[name] else []
    want = HOST_CASES[name] or cfg["frames"] - 1
    for defs, exe in ((), "hostsim_me"), (("-DHM355_HOSTSIM_REVERSE",), "hostsim_me_rev"):
        out = common.build_hostsim(tmp_path, "hostsim_me", *defs, exe=exe)
        r = subprocess.run([str(out)] + args + settings + tail, capture_output=True, text=True)
        assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
        assert f"{want} inter slices" in r.stdout


@pytest.mark.parametrize("name", ["me_full8_ldp_192x128_8b_qp32", "me_tz24_ldp_200x136_8b_qp30"])
def test_hostsim_me_with_the_defaults_does_not_reproduce_the_clip(tmp_path, name):
    """1 / 64 / 4: the fixture discriminates -- the default search arrives at other decisions than the reference did with the clip's settings"""
    _, args = _replay_inputs(tmp_path, name)
    out = common.build_hostsim(tmp_path, "hostsim_me")
    r = subprocess.run([str(out)] + args + [str(v) for v in ME_DEFAULTS], capture_output=True, text=True)
    assert r.returncode == 1 and "MISMATCH" in r.stdout, "the fixture should not be reproduced with the default search"


def test_hostsim_me_with_the_defaults_is_the_default_search(tmp_path):
    """1 / 64 / 4: the same binary reproduces a clip the reference encoded in its default configuration"""
    _, args = _replay_inputs(tmp_path, "ldp_192x128_8b_qp32")
    out = common.build_hostsim(tmp_path, "hostsim_me")
    r = subprocess.run([str(out)] + args + [str(v) for v in ME_DEFAULTS], capture_output=True, text=True)
    assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:]
