"""CPU suite: the fast encoder decisions of hm355_set_fast_decisions (the reference's --ESD / --CFM / --ECU) in the kernel source, on the host
twin tests/hostsim/hostsim_fast.cpp against clips the real reference encoded with the switches (tests/gen_golden_fast.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import common

FAST_P_CASES = ["fast_esd_ldp_192x128_8b_qp32", "fast_cfm_ldp_200x136_8b_qp30", "fast_ecu_ldpwpp_256x136_8b_qp30", "fast_all_aq_ldp_256x136_8b_qp32"]
FAST_CASES = FAST_P_CASES + ["fast_all_ra_192x128_10b_qp32", "fast_all_ldb_200x136_8b_qp30"]


def fast_flags(name):
    g = np.load(os.path.join(common.GOLD, name + ".npz"))
    return tuple(int(g[k]) for k in ("esd", "cfm", "ecu"))


def _replay_inputs(tmp_path, name):
    """the clip, the HMD2 stream of its 'S' / 'F' records and (cu_qp_delta clips) the per-slice QPs for hostsim_fast -> argument list"""
    import hm355
    import hmd2
    import synth
    recs = []
    cfg, slices, _ = common.load_ldp_case(name, recs)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump2.bin"
    synth.write_yuv(str(yuv), w, h, bd, cfg["frames"], cfg["seed"])
    hmd2.write(str(dump), recs)
    args = [str(yuv), str(dump), str(w), str(h), str(bd), str(cfg["wpp"])]
    dqp = None
    if any(r["dqp"] is not None for r in slices):
        n = ((w + 63) // 64) * ((h + 63) // 64)
        dqp = tmp_path / "dqp.bin"
        with open(dqp, "wb") as f:
            for r in slices:
                q = r["dqp"]
                ctu_qp = hm355.aq_ctu_qp(q["activity"], float(q["avg_activity"]), int(q["aq_range"]), int(r["qp"]), bd) if int(q["aq_range"]) > 0 else np.full(n, int(r["qp"]))
                f.write(struct.pack("<i", int(q["dqp_flag_in"])) + np.asarray(ctu_qp).astype(np.int8).tobytes())
    return cfg, args, dqp


def test_fixtures_differ_from_the_reference_without_the_switches():
    """every clip names its switches, has three inter slices or more, and the reference's own decisions change in two inter pictures or more"""
    for name in FAST_CASES:
        g = np.load(os.path.join(common.GOLD, name + ".npz"))
        _, slices, _ = common.load_ldp_case(name)
        diff = g["diff_ctus_vs_off"]
        assert len(diff) == len(slices) and sum(fast_flags(name)) >= 1
        inter = [int(d) for r, d in zip(slices, diff) if int(r["slice_type"]) != 2]
        assert len(inter) >= 3 and sum(d > 0 for d in inter) >= 2, f"{name}: {inter}"


@pytest.mark.parametrize("name", FAST_P_CASES)
def test_hostsim_fast_matches_reference_with_the_switches(tmp_path, name):
    """the kernel source on the host with one lane, forwards and with every lane-parallel loop reversed, with the switches the fixture names:
    every P slice bit for bit (decisions, motion, coefficients, costs, reconstruction) -- and NOT with the switches off"""
    cfg, args, dqp = _replay_inputs(tmp_path, name)
    flags = [str(v) for v in fast_flags(name)]
    tail = [str(dqp)] if dqp else []
    for defs, exe in ((), "hostsim_fast"), (("-DHM355_HOSTSIM_REVERSE",), "hostsim_fast_rev"):
        out = common.build_hostsim(tmp_path, "hostsim_fast", *defs, exe=exe)
        r = subprocess.run([str(out)] + args + flags + tail, capture_output=True, text=True)
        assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
        assert f"{cfg['frames'] - 1} inter slices" in r.stdout
    r = subprocess.run([str(out)] + args + ["0", "0", "0"] + tail, capture_output=True, text=True)
    assert r.returncode == 1 and "MISMATCH" in r.stdout, "the fixture should not be reproduced without its switches"


def test_hostsim_fast_without_switches_is_the_default_search(tmp_path):
    """flags 0/0/0: the same binary reproduces a clip the reference encoded in its default configuration"""
    _, args, _ = _replay_inputs(tmp_path, "ldp_192x128_8b_qp32")
    out = common.build_hostsim(tmp_path, "hostsim_fast")
    r = subprocess.run([str(out)] + args + ["0", "0", "0"], capture_output=True, text=True)
    assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:]
