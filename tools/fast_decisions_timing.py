"""What hm355_set_fast_decisions buys and costs: 1080p low-delay P slices with 4 references (the ldp_p workload of bench.py: independent
streams, WaveFrontSynchro=1, every stream the clip shifted by its own offset) searched with the switches off, with --ESD, --CFM and --ECU alone
and with all three, at each stream count.  Per run: CTU/s from the HIP-event time of the launch, and the summed bits and distortion of the
decisions, so that the rate-distortion price of a speed-up is visible.  With the switches on a P launch runs without wavefront teams, so at
small stream counts the figure contains the loss of the teams.

    fast_decisions_timing.py [--streams 32,320] [--combos off,esd,cfm,ecu,all] [--repeat N] [--lib PATH --label NAME] [--out FILE]
    HM355_FAST=111 fast_decisions_timing.py --bench-c3 [--out FILE]

--lib PATH: another build of libhm355.so (one from before the setter existed included) searches the same jobs with the switches off before and
after this checkout does, an A/B run of the switches-off path in one process.  --bench-c3 runs bench.py's c3 workload with WaveFrontSynchro=1
(one stream, closed loop through hm355_encmain) in this process; the switches come from the environment variable HM355_FAST (<esd><cfm><ecu>), which
hm355_encmain reads when bench.py starts it; bench.py itself is not touched.
Every run is appended to the `runs` list of FILE (default profiles/fast_decisions_timing.json), stamped with hm355_build_id."""
import argparse
import contextlib
import io
import json
import math
import os
import sys
import time

import numpy as np

import _paths
import hm355
import synth

COMBOS = {"off": (0, 0, 0), "esd": (1, 0, 0), "cfm": (0, 1, 0), "ecu": (0, 0, 1), "all": (1, 1, 1)}
W, H, BD, NREF, QP = 1920, 1080, 8, 4, 32


def append_runs(path, runs):
    doc = json.load(open(path)) if os.path.exists(path) else {"tool": "tools/fast_decisions_timing.py", "runs": []}
    doc["runs"] += runs
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def ldp_p_jobs(enc, streams):
    """bench.py run_inter's ldp_p jobs: 4 I-slice reconstructions as references, one P picture per stream"""
    n, qpp = enc.num_ctus, QP + 3
    res = enc.compress([synth.frame(W, H, BD, f, 1234) for f in range(NREF)], QP)
    refs = {f: dict(slice_type=2, rec=res[f][0], pred_mode=np.ones((n, 256), np.uint8), mv=[np.zeros((n, 256, 2), np.int16)] * 2,
                    ref_idx=[np.full((n, 256), -1, np.int8)] * 2, num_ref_idx=(0, 0), ref_poc=np.zeros((2, 16), np.int32),
                    ref_long_term=np.zeros((2, 16), np.int32)) for f in range(NREF)}
    lam = 0.4624 * 2.0 ** ((qpp - 12) / 3.0) * min(4.0, max(2.0, (qpp - 12) / 6.0))
    ref_poc = np.zeros((2, 16), np.int32)
    ref_poc[0, :NREF] = [3, 2, 1, 0]
    sp = dict(slice_type=1, qp=qpp, chroma_weight=hm355.intra_lambda(qpp)[1], poc=NREF, cabac_init_type=1, num_ref_idx=(NREF, 0), ref_poc=ref_poc,
              col_from_l0=1, col_ref_idx=0, tmvp=1, mvd_l1_zero=0, max_merge_cand=5, check_ldc=1,
              lambda_motion_sad=int(math.floor(65536.0 * math.sqrt(lam))), lambda_motion_sse=int(math.floor(65536.0 * lam)))
    sp["lambda"] = lam
    cur0 = synth.frame(W, H, BD, NREF, 1234)

    def shifted(planes, k):
        dx, dy = (24 * k) % W, (8 * k) % H
        return [np.ascontiguousarray(np.roll(np.roll(p, dy >> (1 if i else 0), axis=0), dx >> (1 if i else 0), axis=1)) for i, p in enumerate(planes)]
    return [(shifted(cur0, k), sp, {f: dict(r, rec=shifted(r["rec"], k)) for f, r in refs.items()}) for k in range(streams)]


def time_streams(args, other, build_id, other_id):
    runs = []
    for streams in [int(v) for v in args.streams.split(",")]:
        enc = hm355.Encoder(W, H, BD, 1, max(streams, NREF))
        jobs = ldp_p_jobs(enc, streams)
        encs = {"this checkout": (enc, build_id)}
        order = [("this checkout", c) for c in args.combos.split(",")] * args.repeat
        if other:       # A/B of the switches-off path on the same jobs: the other build before and after this one
            encs[args.label] = (hm355.Encoder(W, H, BD, 1, max(streams, NREF), lib=other), other_id)
            order = [(args.label, "off"), ("this checkout", "off"), (args.label, "off")] + [o for o in order if o[1] != "off"]
        for label, combo in order:
            e, bid = encs[label]
            if label == "this checkout":
                e.set_fast_decisions(*COMBOS[combo])
            t0 = time.perf_counter()
            out = e.compress_inter_batch(jobs)
            call_s = time.perf_counter() - t0
            k, l = hm355.C.c_double(), hm355.C.c_int()
            e.lib.hm355_last_run_info(e.h_, hm355.C.byref(k), hm355.C.byref(l))
            ctus = e.num_ctus * streams
            run = {"workload": f"ldp_p {W}x{H} {BD}-bit, {NREF} references, QP {QP + 3}, WaveFrontSynchro=1", "label": label, "hm355_build_id": bid,
                   "streams": streams, "switches": combo, "ctus": ctus, "kernel_ms": k.value, "ctu_per_s": ctus / (k.value * 1e-3), "call_s": call_s,
                   "bits": int(sum(int(o[1]["total_bits"].sum()) for o in out)), "dist": int(sum(int(o[1]["total_dist"].sum()) for o in out)),
                   "skip": float(np.mean([(o[2]["skip"] != 0).mean() for o in out]))}
            print(json.dumps(run), flush=True)
            runs.append(run)
        for e, _ in encs.values():
            e.close()
    return runs


def bench_c3(build_id):
    flags = os.environ.get("HM355_FAST", "000")             # read by hm355_encmain, which bench.py starts with this process's environment
    assert len(flags) == 3 and set(flags) <= {"0", "1"}, "HM355_FAST=<esd><cfm><ecu>"
    import bench
    argv, sys.argv = sys.argv, ["bench.py", "--workload", "c3", "--gpus", "1", "--steps", "1", "--warmup", "0", "--wpp", "1", "--no-cpu-baseline"]
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            bench.main()
    finally:
        sys.argv = argv
    line = json.loads([l for l in buf.getvalue().splitlines() if l.startswith("{")][-1])
    run = {"workload": "bench.py --workload c3 --wpp 1 (one stream, closed loop)", "label": "this checkout", "hm355_build_id": build_id, "switches": flags, "bench_line": line}
    print(json.dumps(run), flush=True)
    return [run]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="32,320")
    ap.add_argument("--combos", default="off,esd,cfm,ecu,all")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--lib", default=None, help="another build of libhm355.so for the A/B run of the switches-off path")
    ap.add_argument("--label", default="other build", help="what --lib is, e.g. 'parent commit'")
    ap.add_argument("--bench-c3", action="store_true")
    ap.add_argument("--out", default=os.path.join(_paths.ROOT, "profiles", "fast_decisions_timing.json"))
    args = ap.parse_args()
    other, other_id = None, None
    if args.lib:
        os.environ["HM355_OLD_LIB_OK"] = "1"            # a build from before the setter existed is fine: it only runs with the switches off
        other = hm355.load_library(args.lib)
        other_id = other.hm355_build_id().decode()
    build_id = hm355.load_library().hm355_build_id().decode()
    runs = bench_c3(build_id) if args.bench_c3 else time_streams(args, other, build_id, other_id)
    append_runs(args.out, runs)


if __name__ == "__main__":
    main()
