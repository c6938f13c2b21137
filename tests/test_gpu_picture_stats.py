"""GPU suite of the picture statistics (-m gpu): hm355_picture_stats / hm355_picture_stats_run against the reference's own log lines
(tests/golden/pichash_*.npz), against the numpy / hashlib restatement on fresh inputs (tests/picstat_ref.py, pinned by the reference in
tests/test_picture_stats_host.py) and against the finished-picture MD5s of the full-size pins.  Every comparison is for equality."""
import numpy as np
import pytest

import common
import picstat_ref
import synth
from test_picture_stats_host import PICHASH_CASES, load_pichash_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


def assert_stats(got, want, what):
    assert got["ssd"] == want["ssd"], f"{what}: SSD {got['ssd']} != {want['ssd']}"
    assert got["psnr_string"] == want["psnr_string"], f"{what}: PSNR {got['psnr_string']!r} != {want['psnr_string']!r}"
    assert got["mse"] == want["mse"], f"{what}: MSE"
    assert got["digest_string"] == want["digest_string"], f"{what}: digest {got['digest_string']} != {want['digest_string']}"


@pytest.mark.parametrize("name", PICHASH_CASES)
def test_host_buffer_entry_matches_reference_log(hm, name):
    """hm355_picture_stats on every fixture picture, methods 0-3: SSD (against numpy), PSNR string and digest string equal to the reference's log"""
    cfg, pics = load_pichash_case(name)
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], 0, max_batch=1)
    for p in pics:
        ssd = tuple(picstat_ref.ssd(p["org"][k], p["rec"][k], cfg["pad_right"], cfg["pad_bottom"], k > 0)[0] for k in range(3))
        for m in (0, 1, 2, 3):
            got = enc.picture_stats(p["org"], p["rec"], m, cfg["pad_right"], cfg["pad_bottom"])
            what = f"{name} POC {p['poc']} method {m}"
            assert got["ssd"] == ssd, what
            assert got["psnr_string"] == p["psnr"], f"{what}: {got['psnr_string']!r} != {p['psnr']!r}"
            assert got["digest_string"] == (p["digest"][m] if m else ""), f"{what}: {got['digest_string']}"
            assert got["digest_len"] == {0: 0, 1: 16, 2: 2, 3: 4}[m]
    enc.close()


@pytest.mark.parametrize("name", PICHASH_CASES)
def test_device_resident_batch_matches_reference_log(hm, name):
    """all pictures of a clip in different slots, one hm355_picture_stats_run per method; then one call whose descriptors differ in method and
    pads from slot to slot"""
    cfg, pics = load_pichash_case(name)
    n, bd = len(pics), cfg["bit_depth"]
    enc = hm.Encoder(cfg["width"], cfg["height"], bd, 0, max_batch=n)
    for i, p in enumerate(pics):
        enc.upload(i, p["org"]); enc.upload_rec(i, p["rec"])
    for m in (0, 1, 2, 3):
        res = enc.picture_stats_run([dict(hash_method=m, pad_right=cfg["pad_right"], pad_bottom=cfg["pad_bottom"])] * n)
        for p, got in zip(pics, res):
            assert got["psnr_string"] == p["psnr"] and got["digest_string"] == (p["digest"][m] if m else ""), f"{name} POC {p['poc']} method {m}"
    descs = [dict(hash_method=(i + 1) % 4, pad_right=(2 * i) % 8, pad_bottom=(4 * i + 2) % 8) for i in range(n)]
    res = enc.picture_stats_run(descs)
    for i, (p, d, got) in enumerate(zip(pics, descs, res)):
        assert_stats(got, picstat_ref.picture_stats(p["org"], p["rec"], bd, d["hash_method"], d["pad_right"], d["pad_bottom"]), f"{name} slot {i} {d}")
    enc.close()


# width, height, bit depth, pad right, pad bottom, reconstruction ("noise": full-range, independent of the original; "same": the original)
FRESH = [(3840, 2160, 10, 0, 0, "noise"),          # 64-bit SSD, 133 Mbit MD5 length, checksum mask terms up to x >> 8 = 14
         (1920, 1088, 8, 0, 8, "noise"),           # 1080 -> 1088: the bottom pad leaves the SSD and stays in the hash
         (1920, 1088, 8, 0, 0, "same")]            # reconstruction == original: SSD 0, PSNR 999.99


@pytest.mark.parametrize("w,h,bd,pr,pb,kind", FRESH)
def test_fresh_inputs_match_restatement(hm, w, h, bd, pr, pb, kind):
    rng = np.random.default_rng(w + h + bd)
    org = [rng.integers(0, 1 << bd, (h >> (k > 0), w >> (k > 0))).astype(np.uint16) for k in range(3)]
    rec = [p.copy() for p in org] if kind == "same" else [rng.integers(0, 1 << bd, p.shape).astype(np.uint16) for p in org]
    enc = hm.Encoder(w, h, bd, 0, max_batch=1)
    enc.upload(0, org); enc.upload_rec(0, rec)
    for m in (0, 1, 2, 3):
        want = picstat_ref.picture_stats(org, rec, bd, m, pr, pb)
        got, = enc.picture_stats_run([dict(hash_method=m, pad_right=pr, pad_bottom=pb)])
        assert_stats(got, want, f"{w}x{h} {bd}-bit method {m}")
    if kind == "noise":
        assert want["ssd"][0] > 1 << 32                 # the luma SSD needs 64 bits
    else:
        assert got["ssd"] == (0, 0, 0) and got["psnr"] == (999.99, 999.99, 999.99)
    enc.close()


@pytest.mark.parametrize("name", [n for n in common.FULL_CASES if n.startswith("full_c2_") or n.startswith("full_c4_")])
def test_full_size_finished_picture_md5_without_download(hm, name):
    """the I pictures of the full-size pins through the device pipeline as test_full_size_pictures_match_reference_digests runs it (search ->
    deblocking -> SAO), then hm355_picture_stats_run with method 1: the digest is the reference's MD5 of the finished picture (for 10-bit
    pictures common.md5_of of the 16-bit plane is that MD5) and the picture never leaves the device"""
    cfg, pics = common.load_full_case(name)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    assert bd > 8
    enc = hm.Encoder(w, h, bd, cfg["wpp"], max_batch=1)
    rate = np.zeros((3, 8), np.float64)
    for p in pics:
        st, poc, qp = int(p["slice_type"]), int(p["poc"]), int(p["qp"])
        assert st == 2
        enc.upload(0, synth.frame(w, h, bd, poc, cfg["seed"]))
        sl = (hm.SliceDesc * 1)(hm.SliceDesc(2, qp, float(p["lambda"]), float(p["weight_cb"])))
        enc._check(enc.lib.hm355_run(enc.h_, 1, sl), "hm355_run")
        enc.deblock_run([(st, qp, p["ref_poc"])])
        enc.sao_run([dict(qp=qp, cabac_init_type=int(p["cabac_init_type"]), depth=int(p["sao_depth"]), disabled_rate=rate,
                          chroma_weight=float(p["weight_cb"]), **{"lambda": float(p["lambda"])})])
        got, = enc.picture_stats_run([dict(hash_method=1)])
        for c in range(3):
            assert got["digest"][c] == p["final_md5"][c].tobytes(), f"{name} POC {poc}: MD5 of finished plane {c}"
    enc.close()


def test_padded_clip_end_to_end_matches_reference_log(hm):
    """100x60 file frame -> hm355_upload_file_frames into a 104x64 context -> search -> deblocking -> SAO -> hm355_picture_stats_run with the pads:
    the reference's log line of POC 0 (slice parameters from the fixture's 'S' record)"""
    name = "pichash_pad_100x60_8b"
    cfg, pics = load_pichash_case(name)
    g = np.load(common.GOLD + "/" + name + ".npz")
    s = {k: g[f"s0_{k}"][()] for k in common._S_KEYS}
    p = pics[0]
    assert p["poc"] == 0 and int(s["slice_type"]) == 2
    sw, sh, bd, qp = cfg["source_width"], cfg["source_height"], cfg["bit_depth"], int(s["qp"])
    raw = b"".join(pl.astype(np.uint8).tobytes() for pl in synth.frame(sw, sh, bd, 0, cfg["seed"]))
    enc = hm.Encoder(cfg["width"], cfg["height"], bd, 0, max_batch=1)
    enc.upload_file_frames([raw], sw, sh, bd)
    sl = (hm.SliceDesc * 1)(hm.SliceDesc(2, qp, float(s["lambda"]), float(s["weight_cb"])))
    enc._check(enc.lib.hm355_run(enc.h_, 1, sl), "hm355_run")
    enc.deblock_run([(2, qp, None)])
    enc.sao_run([dict(qp=qp, cabac_init_type=int(s["cabac_init_type"]), depth=int(g["s0_depth"]), disabled_rate=np.zeros((3, 8), np.float64),
                      chroma_weight=float(s["weight_cb"]), **{"lambda": float(s["lambda"])})])
    for m in (1, 2, 3):
        got, = enc.picture_stats_run([dict(hash_method=m, pad_right=cfg["pad_right"], pad_bottom=cfg["pad_bottom"])])
        assert got["psnr_string"] == p["psnr"], f"method {m}: {got['psnr_string']!r} != {p['psnr']!r}"
        assert got["digest_string"] == p["digest"][m], f"method {m}: {got['digest_string']} != {p['digest'][m]}"
    enc.close()


def test_bad_arguments_are_rejected_and_the_context_stays_usable(hm):
    w, h, bd = 200, 136, 8
    org, rec = synth.frame(w, h, bd, 0, 5), synth.frame(w, h, bd, 1, 5)
    enc = hm.Encoder(w, h, bd, 0, max_batch=2)
    enc.upload(0, org); enc.upload_rec(0, rec)
    want = picstat_ref.picture_stats(org, rec, bd, 2, 8, 8)
    C = hm.C

    def rc_of(n, **kw):
        arr = (hm.PicStatDesc * max(n, 1))()
        for k in range(max(n, 1)):
            arr[k].hash_method, arr[k].pad_right, arr[k].pad_bottom = kw.get("hash_method", 0), kw.get("pad_right", 0), kw.get("pad_bottom", 0)
        return enc.lib.hm355_picture_stats_run(enc.h_, n, arr)

    bad = [(0, {}), (3, {}), (-1, {}), (1, dict(hash_method=4)), (1, dict(hash_method=-1)), (1, dict(pad_right=-2)), (1, dict(pad_bottom=-2)),
           (1, dict(pad_right=3)), (1, dict(pad_bottom=1)), (1, dict(pad_right=w)), (1, dict(pad_bottom=h)), (1, dict(pad_right=w + 8))]
    for n, kw in bad:
        assert rc_of(n, **kw) == -1, (n, kw)            # HM355_ERR_ARG
        got, = enc.picture_stats_run([dict(hash_method=2, pad_right=8, pad_bottom=8)])
        assert_stats(got, want, f"after the rejected call {n} {kw}")
    assert enc.lib.hm355_picture_stats_run(enc.h_, 1, None) == -1
    d = hm.PicStatDesc()
    assert enc.lib.hm355_picture_stats(enc.h_, C.byref(d), None, None) == -1
    enc.close()


def test_statistics_change_nothing(hm):
    """the reconstruction and the originals are the same before and after, and the next hm355_run on the context still reproduces its fixture"""
    name = "c1_416x240_8b_qp32"
    cfg, frames = common.load_case(name)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    enc = hm.Encoder(w, h, bd, cfg["wpp"], max_batch=1)
    planes = synth.frame(w, h, bd, 0, cfg["seed"])
    enc.upload(0, planes)
    enc.run(1, cfg["qp"])
    rec0, ctus0, _ = enc.download(0)
    org0 = enc.download_org(0)
    for m in (0, 1, 2, 3):
        got, = enc.picture_stats_run([dict(hash_method=m, pad_right=8, pad_bottom=8)])
        assert_stats(got, picstat_ref.picture_stats(planes, rec0, bd, m, 8, 8), f"{name} method {m}")
    rec1, ctus1, _ = enc.download(0)
    org1 = enc.download_org(0)
    for k in range(3):
        assert np.array_equal(rec0[k], rec1[k]) and np.array_equal(org0[k], org1[k])
    assert ctus0.tobytes() == ctus1.tobytes()
    enc.run(1, cfg["qp"])
    rec2, ctus2, _ = enc.download(0)
    common.assert_ctus_equal(ctus2, frames[0][0], name, (w, h))
    common.assert_rec_equal(rec2, frames[0][1], w, h, name)
    enc.close()


@pytest.mark.parametrize("name,method", [(common.LDP_CASES[2], 1), (common.B_CASES[1], 2), (common.B_CASES[0], 3)])     # low-delay P, low-delay B, random access
def test_cpp_host_mirror_writes_psnr_and_digest(tmp_path, name, method):
    """hm355_encmain with its hash=N argument on clips of test_cpp_host_mirror_inter_configurations: for every picture in coding order the PSNR and
    digest text of the reference's log line.  Expected text: the restatement on the fixture's finished pictures (which that test proves the mirror
    reproduces) against the synth originals.  The dump and the slice data are byte for byte what a run without the argument writes."""
    import os, subprocess
    cfg, slices, finals = common.load_ldp_case(name)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    yuv = tmp_path / "in.yuv"
    synth.write_yuv(str(yuv), w, h, bd, cfg["frames"], cfg["seed"])
    exe = os.path.join(common.ROOT, "hm-16.2_amd", "hm355_encmain")
    mode = "ldb" if name.startswith("ldb") else ("ra" if "ra_" in name else "ldp")
    base = [exe, str(yuv), str(w), str(h), str(bd), str(cfg["frames"]), str(int(slices[0]["qp"])), str(cfg["wpp"])]
    plain, hashed = tmp_path / "plain.bin", tmp_path / "hashed.bin"
    subprocess.run(base + [str(plain), mode], check=True)
    subprocess.run(base + [str(hashed), mode, f"hash={method}"], check=True)
    assert open(plain, "rb").read() == open(hashed, "rb").read()
    assert open(str(plain) + ".bits", "rb").read() == open(str(hashed) + ".bits", "rb").read()
    assert not os.path.exists(str(plain) + ".picstat")
    lines = open(str(hashed) + ".picstat").read().split("\n")
    assert lines[-1] == "" and len(lines) == len(slices) + 1
    tag = {1: "MD5", 2: "CRC", 3: "Checksum"}[method]
    for r, line in zip(slices, lines):
        poc = int(r["poc"])
        want = picstat_ref.picture_stats(synth.frame(w, h, bd, poc, cfg["seed"]), finals[poc]["rec"], bd, method)
        assert line == want["psnr_string"] + f" [{tag}:{want['digest_string']}]", f"{name} POC {poc}: {line!r}"
