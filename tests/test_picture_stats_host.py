"""Picture statistics (PSNR, decoded picture hash) without a GPU: the numpy / hashlib restatement (tests/picstat_ref.py) and the CPU twin of the
kernels (tests/hostsim/hostsim_picstat.cpp, the arithmetic of hm-16.2_amd/csrc/hm355_picstat.h) against the reference's own log lines
(tests/golden/pichash_*.npz, tests/gen_golden_pichash.py), and the C ABI's declarations and exports.  Every comparison is for equality."""
import os
import re
import subprocess

import numpy as np
import pytest

import common
import picstat_ref

PICHASH_CASES = ["pichash_ldp_200x136_8b", "pichash_ra_136x72_10b", "pichash_ldp_328x264_8b", "pichash_pad_100x60_8b"]


def load_pichash_case(name):
    """-> (cfg, [picture dict: poc, org, rec (uint16 planes of the coded size), psnr (string), digest {method: string}] in coding order)"""
    g = np.load(os.path.join(common.GOLD, name + ".npz"))
    cfg = {k: int(g[k]) for k in ("width", "height", "source_width", "source_height", "pad_right", "pad_bottom", "bit_depth", "frames", "seed", "qp")}
    pics = []
    for i in range(cfg["frames"]):
        pics.append({"poc": int(g[f"p{i}_poc"]), "org": [g[f"p{i}_org{k}"].astype(np.uint16) for k in range(3)],
                     "rec": [g[f"p{i}_rec{k}"].astype(np.uint16) for k in range(3)], "psnr": str(g[f"p{i}_psnr"]),
                     "digest": {m: str(g[f"p{i}_digest{m}"]) for m in (1, 2, 3)}})
    return cfg, pics


def test_fixtures_cover_the_cases_the_kernels_must_handle():
    sizes = {n: load_pichash_case(n)[0] for n in PICHASH_CASES}
    assert any(c["width"] % 64 and c["bit_depth"] == 8 for c in sizes.values())                     # slot stride != width
    assert any(c["bit_depth"] == 10 for c in sizes.values())
    assert any(c["width"] > 256 and c["height"] > 256 for c in sizes.values())                     # x >> 8, y >> 8 of the checksum mask
    assert any(c["pad_right"] > 0 and c["pad_bottom"] > 0 for c in sizes.values())


@pytest.mark.parametrize("name", PICHASH_CASES)
def test_restatement_reproduces_the_reference_log(name):
    cfg, pics = load_pichash_case(name)
    for p in pics:
        for m in (0, 1, 2, 3):
            got = picstat_ref.picture_stats(p["org"], p["rec"], cfg["bit_depth"], m, cfg["pad_right"], cfg["pad_bottom"])
            assert got["psnr_string"] == p["psnr"], (name, p["poc"], m)
            if m:
                assert got["digest_string"] == p["digest"][m], (name, p["poc"], m)
        for k in range(3):                         # the fast CRC is the reference's bit-by-bit loop
            assert picstat_ref.crc(p["rec"][k], cfg["bit_depth"]) == picstat_ref.crc_bitwise(p["rec"][k], cfg["bit_depth"])


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    return common.build_hostsim(tmp_path_factory.mktemp("picstat"), "hostsim_picstat")


WALKS = [(64, 0), (64, 1), (24, 0), (24, 1)]       # (samples per CRC chunk, walk the partition backwards)


def run_twin(exe, tmp_path, org, rec, bit_depth, method, pad_right, pad_bottom, chunk, reverse):
    h, w = org[0].shape
    path = tmp_path / "pic.bin"
    with open(path, "wb") as f:
        f.write(np.array([w, h, bit_depth, pad_right, pad_bottom, method], "<i4").tobytes())
        for p in list(org) + list(rec):
            f.write(np.ascontiguousarray(p, "<u2").tobytes())
    out = subprocess.run([str(exe), str(path), str(chunk), str(reverse)], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout.splitlines()
    assert out[0].startswith("ssd ") and out[1].startswith("psnr") and out[2].startswith("mse ") and out[3].startswith("digest ")
    return {"ssd": tuple(int(v) for v in out[0].split()[1:]), "psnr_string": out[1][4:], "mse": tuple(float.fromhex(v) for v in out[2].split()[1:]),
            "digest_string": out[3][7:]}


@pytest.mark.parametrize("name", PICHASH_CASES)
def test_twin_reproduces_the_reference_log(twin, tmp_path, name):
    cfg, pics = load_pichash_case(name)
    for p in pics:
        ssd = tuple(picstat_ref.ssd(p["org"][k], p["rec"][k], cfg["pad_right"], cfg["pad_bottom"], k > 0)[0] for k in range(3))
        for m in (0, 1, 2, 3):
            for chunk, reverse in WALKS:
                got = run_twin(twin, tmp_path, p["org"], p["rec"], cfg["bit_depth"], m, cfg["pad_right"], cfg["pad_bottom"], chunk, reverse)
                assert got["psnr_string"] == p["psnr"], (name, p["poc"], m, chunk, reverse)
                assert got["ssd"] == ssd
                assert got["digest_string"] == (p["digest"][m] if m else ""), (name, p["poc"], m, chunk, reverse)


# width, height, bit depth, pad right, pad bottom, reconstruction: "noise" (full-range, independent of the original) or "same" (== original)
RANDOM_PLANES = [(200, 136, 8, 0, 0, "noise"), (136, 72, 10, 0, 0, "noise"), (104, 64, 8, 4, 4, "noise"), (520, 264, 10, 6, 2, "noise"),
                 (520, 264, 8, 0, 8, "noise"), (72, 40, 10, 0, 0, "same"), (8, 8, 8, 0, 0, "noise")]


def random_picture(w, h, bd, kind, seed):
    rng = np.random.default_rng(seed)
    org = [rng.integers(0, 1 << bd, (h >> (k > 0), w >> (k > 0))).astype(np.uint16) for k in range(3)]
    rec = [p.copy() for p in org] if kind == "same" else [rng.integers(0, 1 << bd, p.shape).astype(np.uint16) for p in org]
    return org, rec


@pytest.mark.parametrize("w,h,bd,pr,pb,kind", RANDOM_PLANES)
def test_twin_equals_the_restatement_on_random_planes(twin, tmp_path, w, h, bd, pr, pb, kind):
    org, rec = random_picture(w, h, bd, kind, 1000 + w + h + bd)
    for m in (0, 1, 2, 3):
        want = picstat_ref.picture_stats(org, rec, bd, m, pr, pb)
        for chunk, reverse in WALKS:
            got = run_twin(twin, tmp_path, org, rec, bd, m, pr, pb, chunk, reverse)
            for k in ("ssd", "psnr_string", "mse", "digest_string"):
                assert got[k] == want[k], (k, m, chunk, reverse)
    if kind == "same":
        assert want["ssd"] == (0, 0, 0) and want["psnr_string"] == " [Y 999.9900 dB    U 999.9900 dB    V 999.9900 dB]"


def test_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(common.ROOT, "include", "hm355.h")).read()
    lib = os.path.join(common.ROOT, "hm-16.2_amd", "libhm355.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build())"
    syms = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout
    for name in ("hm355_picture_stats_run", "hm355_picture_stats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/hm355.h"
        assert re.search(r"\sT\s+" + name + r"$", syms, re.M), f"{name} is not exported by libhm355.so"
    assert "hm355_picstat_desc" in hdr
