"""Picture statistics on the device against the only route the library offered before them, in one run on one box: for 1, 64 and 192 resident
3840x2160 10-bit pictures, hm355_picture_stats_run with hash methods 0-3 (HIP-event time of the call's launches, wall time of the call) and,
beside it, hm355_download of the reconstruction + hm355_download_org followed by numpy SSD / checksum, binascii's table-driven CRC and
hashlib.md5 on one host core.  The host route is serial per picture, so it is measured on the first HOST_SAMPLE pictures and scaled to the
batch.  The launches of a call share one pair of events: method 0 is hm355_picstat_kernel alone, methods 2 and 1 add hm355_crc_kernel /
hm355_md5_kernel behind it, so their own time is the difference to method 0.  Prints one JSON line (profiles/picstat_timing.json)."""
import json
import sys
import time

import numpy as np

import _paths  # noqa: F401
import hm355
import picstat_ref

W, H, BD = 3840, 2160, 10
HBM_PEAK_GBS = 8000.0
HOST_SAMPLE = 4
BATCHES = [int(v) for v in sys.argv[1:]] or [1, 64, 192]


def main():
    rng = np.random.default_rng(7)
    org = [rng.integers(0, 1 << BD, (H >> (k > 0), W >> (k > 0))).astype(np.uint16) for k in range(3)]
    rec = [np.clip(p.astype(np.int32) + rng.integers(-6, 7, p.shape), 0, (1 << BD) - 1).astype(np.uint16) for p in org]
    plane_bytes = W * H * 3 // 2 * 2
    out = {"tool": "tools/picstat_timing.py", "hm355_build_id": hm355.load_library().hm355_build_id().decode(), "picture": f"{W}x{H} {BD}-bit 4:2:0",
           "hbm_peak_gbs": HBM_PEAK_GBS, "host_sample_pictures": HOST_SAMPLE, "batches": []}
    want = {m: picstat_ref.picture_stats(org, rec, BD, m) for m in range(4)}
    for n in BATCHES:
        enc = hm355.Encoder(W, H, BD, 1, n)
        for i in range(n):
            enc.upload(i, org); enc.upload_rec(i, rec)
        row = {"pictures": n, "device": {}, "host_route": {}}
        for m in range(4):
            descs = [dict(hash_method=m)] * n
            enc.picture_stats_run(descs)                                  # warm-up (first-use allocations)
            best_wall, best_ev = 1e30, 1e30
            for _ in range(3):
                t0 = time.perf_counter()
                res = enc.picture_stats_run(descs)
                wall = (time.perf_counter() - t0) * 1e3
                ms, launches = hm355.C.c_double(), hm355.C.c_int()
                enc.lib.hm355_last_run_info(enc.h_, hm355.C.byref(ms), hm355.C.byref(launches))
                best_wall, best_ev = min(best_wall, wall), min(best_ev, ms.value)
            assert all(r["ssd"] == want[m]["ssd"] and r["digest_string"] == want[m]["digest_string"] for r in res)
            d = {"launches": launches.value, "event_ms": best_ev, "wall_ms": best_wall}
            if m in (0, 3):                                               # the one-pass kernel alone: original + reconstruction read once
                d["algorithmic_gbs"] = 2 * plane_bytes * n / (best_ev * 1e-3) / 1e9
                d["frac_of_hbm_peak"] = d["algorithmic_gbs"] / HBM_PEAK_GBS
            row["device"][str(m)] = d
        k = min(n, HOST_SAMPLE)
        t0 = time.perf_counter()
        pics = []
        for i in range(k):
            r, _, _ = enc.download(i, want_ctus=False)
            pics.append((enc.download_org(i), r))
        copy_ms = (time.perf_counter() - t0) * 1e3
        for m in range(4):
            t0 = time.perf_counter()
            for o, r in pics:
                got = picstat_ref.picture_stats(o, r, BD, m)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert got["ssd"] == want[m]["ssd"] and got["digest_string"] == want[m]["digest_string"]
            row["host_route"][str(m)] = {"download_ms": copy_ms * n / k, "compute_ms_one_core": host_ms * n / k, "wall_ms": (copy_ms + host_ms) * n / k}
        out["batches"].append(row)
        enc.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
