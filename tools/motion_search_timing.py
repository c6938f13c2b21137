"""What hm355_set_motion_search costs: 1080p low-delay P slices with 4 references (the ldp_p workload of bench.py: independent streams,
WaveFrontSynchro=1, every stream the clip shifted by its own offset) searched with the default TZ search (1 / 64 / 4) and with the full search
(fast_search 0) at each range, at each stream count.  Per run: CTU/s from the HIP-event time of the launch, and the summed bits and distortion
of the decisions.  With fast_search 0 a P launch runs without wavefront teams, so at small stream counts the figure contains their loss.

    motion_search_timing.py [--streams 32,320] [--settings tz64,full8,full16,full64] [--repeat N] [--lib PATH --label NAME] [--out FILE]
    motion_search_timing.py --cpu-reference [--settings ...] [--out FILE]

--lib PATH: another build of libhm355.so (one from before the setter existed included) searches the same jobs with the default search before
and after this checkout does, an A/B run of the default path in one process.
--cpu-reference: no GPU; the reference encoder on one host core with the same FastSearch / SearchRange, through bench.py's cpu_baseline_inter
(its bounded sample of the benched clip), one record per setting.
Every run is appended to the `runs` list of FILE (default profiles/motion_search_timing.json), stamped with hm355_build_id."""
import argparse
import json
import os
import re
import time

import numpy as np

import _paths
import hm355
from fast_decisions_timing import BD, H, NREF, QP, W, ldp_p_jobs

SETTINGS = {"tz64": (1, 64, 4), "tz16": (1, 16, 4), "tz256": (1, 256, 4), "full8": (0, 8, 4), "full16": (0, 16, 4), "full32": (0, 32, 4), "full64": (0, 64, 4)}
WORKLOAD = f"ldp_p {W}x{H} {BD}-bit, {NREF} references, QP {QP + 3}, WaveFrontSynchro=1"


def append_runs(path, runs):
    doc = json.load(open(path)) if os.path.exists(path) else {"tool": "tools/motion_search_timing.py", "runs": []}
    doc["runs"] += runs
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def time_streams(args, other, build_id, other_id):
    for streams in [int(v) for v in args.streams.split(",")]:
        enc = hm355.Encoder(W, H, BD, 1, max(streams, NREF))
        jobs = ldp_p_jobs(enc, streams)
        encs = {"this checkout": (enc, build_id)}
        order = [("this checkout", s) for s in args.settings.split(",")] * args.repeat
        if other:       # A/B of the default path on the same jobs: the other build before and after this one
            encs[args.label] = (hm355.Encoder(W, H, BD, 1, max(streams, NREF), lib=other), other_id)
            order = [(args.label, "tz64"), ("this checkout", "tz64"), (args.label, "tz64")] * args.repeat + [o for o in order if o[1] != "tz64"]
        for label, setting in order:
            e, bid = encs[label]
            if label == "this checkout":
                e.set_motion_search(*SETTINGS[setting])
            t0 = time.perf_counter()
            out = e.compress_inter_batch(jobs)
            call_s = time.perf_counter() - t0
            k, l = hm355.C.c_double(), hm355.C.c_int()
            e.lib.hm355_last_run_info(e.h_, hm355.C.byref(k), hm355.C.byref(l))
            ctus = e.num_ctus * streams
            run = {"workload": WORKLOAD, "label": label, "hm355_build_id": bid, "streams": streams, "setting": setting,
                   "fast_search,search_range,bipred_search_range": SETTINGS[setting], "ctus": ctus, "kernel_ms": k.value,
                   "ctu_per_s": ctus / (k.value * 1e-3), "call_s": call_s,
                   "bits": int(sum(int(o[1]["total_bits"].sum()) for o in out)), "dist": int(sum(int(o[1]["total_dist"].sum()) for o in out)),
                   "skip": float(np.mean([(o[2]["skip"] != 0).mean() for o in out]))}
            print(json.dumps(run), flush=True)
            append_runs(args.out, [run])                  # at once: a long full-search run that is cut short does not take the others with it
        for e, _ in encs.values():
            e.close()


def cpu_reference(args, build_id):
    """bench.py's cpu_baseline_inter with the FastSearch / SearchRange lines of its configuration text replaced (bench.py itself is not touched)"""
    import bench
    text = bench.REF_CFG
    try:
        for setting in args.settings.split(","):
            fs, sr, _ = SETTINGS[setting]
            bench.REF_CFG = re.sub(r"(?m)^SearchRange\s*:.*$", f"SearchRange : {sr}", re.sub(r"(?m)^FastSearch\s*:.*$", f"FastSearch : {fs}", text))
            cb = bench.cpu_baseline_inter("ldp_p", QP, W, H)
            assert cb, "the reference encoder is not built"
            run = {"workload": WORKLOAD, "label": "reference encoder, one host core", "hm355_build_id": build_id, "setting": setting,
                   "fast_search,search_range,bipred_search_range": SETTINGS[setting], "ctu_per_s": cb["value"], "sample": cb["sample"]}
            print(json.dumps(run), flush=True)
            append_runs(args.out, [run])
    finally:
        bench.REF_CFG = text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="32,320")
    ap.add_argument("--settings", default="tz64,full8,full16,full64")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--lib", default=None, help="another build of libhm355.so for the A/B run of the default path")
    ap.add_argument("--label", default="other build", help="what --lib is, e.g. 'parent commit'")
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(_paths.ROOT, "profiles", "motion_search_timing.json"))
    args = ap.parse_args()
    other, other_id = None, None
    if args.lib:
        os.environ["HM355_OLD_LIB_OK"] = "1"            # a build from before the setter existed is fine: it only runs the default search
        other = hm355.load_library(args.lib)
        other_id = other.hm355_build_id().decode()
    build_id = hm355.load_library().hm355_build_id().decode()
    if args.cpu_reference:
        cpu_reference(args, build_id)
    else:
        time_streams(args, other, build_id, other_id)


if __name__ == "__main__":
    main()
