"""Fixtures for the picture statistics (PSNR and the decoded picture hash) from the REAL reference encoder: tests/golden/pichash_*.npz.

Every clip is encoded three times by oracle/_ref/hm_dump enc2 with --SEIDecodedPictureHash=1, 2 and 3.  The `POC ...` lines of the encoder's
log carry the PSNR of xCalculateAddPSNR and the digest of the finished picture; the same run's 'F' records carry the finished picture itself and
the input file the originals.  Stored per picture (coding order): original planes (padded by edge repetition to the coded size, as the ingest
does; the pad area enters no result), finished planes, and for each method the PSNR string and the digest string exactly as logged.  Before
saving, the three runs must agree in bits, PSNR and finished planes of every picture.

Usage: python tests/gen_golden_pichash.py   (needs the reference tree to build oracle/_ref/hm_dump)"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "hm-16.2_amd"), os.path.dirname(os.path.abspath(__file__))]
import common  # noqa: E402
import hmd2  # noqa: E402
import synth  # noqa: E402

HM_DUMP = os.path.join(ROOT, "oracle", "_ref", "hm_dump")
REF_CFG = "/root/reference/cfg"
GOLD = os.path.join(ROOT, "tests", "golden")

# name, cfg file, source width, source height, bit depth, frames, qp, seed, conformance window mode
CASES = [
    ("pichash_ldp_200x136_8b", "encoder_lowdelay_P_main.cfg", 200, 136, 8, 3, 32, 1234, 0),        # slot stride != width
    ("pichash_ra_136x72_10b", "encoder_randomaccess_main10.cfg", 136, 72, 10, 9, 32, 4321, 0),      # one GOP: I, P-like, B
    ("pichash_ldp_328x264_8b", "encoder_lowdelay_P_main.cfg", 328, 264, 8, 2, 34, 77, 0),           # x >> 8 and y >> 8 in the checksum mask
    ("pichash_pad_100x60_8b", "encoder_lowdelay_P_main.cfg", 100, 60, 8, 3, 30, 99, 1),             # 104x64 coded: PSNR excludes the pad, the hash includes it
]
LINE = re.compile(r"^POC\s+(\d+)\s.*?\)\s+(\d+) bits (\[Y [^\]]*\])(.*)$")
HASH = re.compile(r"\[(MD5|CRC|Checksum):([0-9a-f,]+)\]")


def run_case(name, cfgfile, w, h, bd, nf, qp, seed, conf):
    cw, ch = ((w + 7) // 8 * 8, (h + 7) // 8 * 8) if conf else (w, h)
    out = {"width": cw, "height": ch, "source_width": w, "source_height": h, "pad_right": cw - w, "pad_bottom": ch - h, "bit_depth": bd,
           "frames": nf, "seed": seed, "qp": qp}
    per_method = {}
    with tempfile.TemporaryDirectory() as td:
        yuv = os.path.join(td, "in.yuv")
        synth.write_yuv(yuv, w, h, bd, nf, seed)
        for m in (1, 2, 3):
            dump = os.path.join(td, f"dump{m}.bin")
            cmd = [HM_DUMP, "enc2", "-c", os.path.join(REF_CFG, cfgfile), "-i", yuv, "-wdt", str(w), "-hgt", str(h), "-fr", "50", "-f", str(nf),
                   f"--InputBitDepth={bd}", "-q", str(qp), "-b", os.path.join(td, "o.bin"), "-o", os.path.join(td, "r.yuv"),
                   f"--ConformanceWindowMode={conf}", f"--SEIDecodedPictureHash={m}", "--", dump]
            log = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, universal_newlines=True).stdout
            lines = []
            for ln in log.splitlines():
                g = LINE.match(ln)
                if g:
                    hm = HASH.search(g.group(4))
                    assert hm and hm.group(1) == {1: "MD5", 2: "CRC", 3: "Checksum"}[m], ln
                    lines.append((int(g.group(1)), int(g.group(2)), " " + g.group(3), hm.group(2)))
            recs = hmd2.parse(dump, cw, ch)           # the 'F' record holds the padded picture
            per_method[m] = (lines, {r["poc"]: r for r in recs if r["tag"] == "F"}, [r for r in recs if r["tag"] == "S"])
    lines1, finals1, slices1 = per_method[1]
    assert len(lines1) == nf, (name, len(lines1))
    for m in (2, 3):                                   # the digest (and the [ET ..] field) is all that may differ between the runs
        lines, finals, _ = per_method[m]
        assert [(a[0], a[1], a[2]) for a in lines] == [(a[0], a[1], a[2]) for a in lines1], name
        for poc in finals1:
            assert all(np.array_equal(finals[poc]["rec"][k], finals1[poc]["rec"][k]) for k in range(3)), name
    store = np.uint8 if bd == 8 else np.uint16
    for i, (poc, bits, psnr, _) in enumerate(lines1):
        org = synth.frame(w, h, bd, poc, seed)
        for k in range(3):
            sw, sh = org[k].shape[1], org[k].shape[0]
            o = np.pad(org[k], ((0, (ch >> (k > 0)) - sh), (0, (cw >> (k > 0)) - sw)), mode="edge")
            out[f"p{i}_org{k}"] = o.astype(store)
            out[f"p{i}_rec{k}"] = finals1[poc]["rec"][k].astype(store)
        out[f"p{i}_poc"] = np.array(poc); out[f"p{i}_bits"] = np.array(bits); out[f"p{i}_psnr"] = np.array(psnr)
        for m in (1, 2, 3):
            out[f"p{i}_digest{m}"] = np.array(per_method[m][0][i][3])
        print(name, "POC", poc, bits, "bits", psnr, per_method[1][0][i][3], per_method[2][0][i][3], per_method[3][0][i][3], flush=True)
    if conf:                                           # the slice parameters of POC 0: the clip also runs end to end through the device pipeline
        s = [r for r in slices1 if r["poc"] == 0][0]
        for k in common._S_KEYS:
            out[f"s0_{k}"] = np.array(s[k])
        out["s0_depth"] = np.array(s["depth"])
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 775 * 1024, (name, os.path.getsize(path))


if __name__ == "__main__":
    for c in CASES:
        if "--only" in sys.argv and c[0] != sys.argv[sys.argv.index("--only") + 1]:
            continue
        run_case(*c)
