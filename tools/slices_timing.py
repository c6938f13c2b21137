"""What slices buy a picture coded without WaveFrontSynchro: 1080p low-delay P (encoder_lowdelay_P_main, 4 references, SearchRange 64,
WaveFrontSynchro=0 -- BASELINE configs[2] as stated, the shape of `bench.py --workload c3`) with one slice, with --SliceMode=1 --SliceArgument=120
(30 x 17 CTUs: 5 slices, the last of 30 CTUs) and with SliceArgument=30 (17 slices, one per CTU row).  The set-up is that of tools/tiles_timing.py.

    slices_timing.py [--args 0,120,30] [--steps N] [--streams 32] [--stream-args 0,30] [--cpu-reference] [--out FILE]

One stream: closed loop through the C++ host mirror (hm355_encmain ... ldp slices=N: search -> deblocking -> SAO -> slice data -> device-resident
reference per picture); per argument the CTU/s and ms per P picture of the search launches (HIP events) and the picture's wall time.  The launch of
one picture runs as teams of nine wavefronts, slices + 2 workgroups (hm355_plan_launch).
--streams S: S such streams in one launch (bench.py's ldp_p jobs on a context without WaveFrontSynchro: one P picture per stream on four
I-picture references), with the launch shape the library reports.
--cpu-reference: no GPU; the reference encoder on one host core with the same slice options (oracle/_ref/hm_encoder, as bench.py's cpu_baseline does
it: 'Total Time' of 1 + n pictures minus the I picture alone).
Argument 0 stands for one slice.  Every run is appended to the `runs` list of FILE (default profiles/slices_timing.json), stamped with hm355_build_id."""
import argparse
import json
import os
import subprocess
import tempfile
import time

import _paths
import hm355
import synth
from fast_decisions_timing import BD, H, NREF, QP, W, ldp_p_jobs

W_CTU, H_CTU = (W + 63) // 64, (H + 63) // 64
WORKLOAD = f"encoder_lowdelay_P_main, synthetic {W}x{H} {BD}-bit, {NREF} references, SearchRange 64, QP {QP}, WaveFrontSynchro=0"


def append_runs(path, runs):
    doc = json.load(open(path)) if os.path.exists(path) else {"tool": "tools/slices_timing.py", "runs": []}
    doc["runs"] += runs
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


def partition(arg):
    """the first CTUs of SliceMode=1 without WaveFrontSynchro, and the size of the largest slice, which bounds the picture"""
    n = W_CTU * H_CTU
    first = list(range(0, n, arg)) if arg else [0]
    return first, max(b - a for a, b in zip(first, first[1:] + [n]))


def one_stream(args, build_id):
    exe = os.path.join(_paths.ROOT, "hm-16.2_amd", "hm355_encmain")
    nf = 1 + args.steps
    with tempfile.TemporaryDirectory() as td:
        yuv = os.path.join(td, "in.yuv")
        synth.write_yuv(yuv, W, H, BD, nf, 1234)
        for arg in (int(v) for v in args.args.split(",")):
            first, largest = partition(arg)
            cmd = [exe, yuv, str(W), str(H), str(BD), str(nf), str(QP), "0", os.path.join(td, "dump.bin"), "ldp"] + ([f"slices={arg}"] if arg else [])
            p = subprocess.run(cmd, env=dict(os.environ, HM355_TIMING="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=True)
            pics = [json.loads(l) for l in p.stderr.decode().splitlines() if l.startswith("{")]
            timed = [x for x in pics if x["slice_type"] != 2]
            kernel_ms = sum(x["search_kernel_ms"] for x in timed)
            n = W_CTU * H_CTU
            run = {"workload": WORKLOAD + ", ONE stream in closed loop", "hm355_build_id": build_id, "slice_argument": arg, "slices": len(first), "largest_slice_ctus": largest,
                   "streams": 1, "p_pictures": len(timed), "ctu_per_s": n * len(timed) / (kernel_ms * 1e-3), "search_ms_per_picture": kernel_ms / len(timed),
                   "picture_wall_ms": sum(x["picture_wall_ms"] for x in timed) / len(timed), "i_picture_search_ms": pics[0]["search_kernel_ms"],
                   "launch": {"kernel": "team", "waves": 9, "workgroups": min(len(first) + 2, n)}, "bits": [x["bits"] for x in pics]}
            print(json.dumps(run), flush=True)
            append_runs(args.out, [run])


def many_streams(args, build_id):
    streams = args.streams
    enc = hm355.Encoder(W, H, BD, 0, max(streams, NREF))
    jobs = ldp_p_jobs(enc, streams)
    for arg in (int(v) for v in args.stream_args.split(",")):
        first, largest = partition(arg)
        enc.set_slices(first)
        t0 = time.perf_counter()
        out = enc.compress_inter_batch(jobs)
        call_s = time.perf_counter() - t0
        k, l = hm355.C.c_double(), hm355.C.c_int()
        enc.lib.hm355_last_run_info(enc.h_, hm355.C.byref(k), hm355.C.byref(l))
        ctus = enc.num_ctus * streams
        run = {"workload": WORKLOAD + f", {streams} independent streams in one launch, QP {QP + 3}", "hm355_build_id": build_id, "slice_argument": arg, "slices": len(first),
               "largest_slice_ctus": largest, "streams": streams, "ctus": ctus, "kernel_ms": k.value, "ctu_per_s": ctus / (k.value * 1e-3), "call_s": call_s,
               "launch": enc.last_launch_shape(), "bits": int(sum(int(o[1]["total_bits"].sum()) for o in out))}
        print(json.dumps(run), flush=True)
        append_runs(args.out, [run])
    enc.close()


def cpu_reference(args, build_id):
    import bench
    enc_bin = os.path.join(_paths.ROOT, "oracle", "_ref", "hm_encoder")
    assert os.path.exists(enc_bin), "the reference encoder is not built"
    keep = ("MaxCUWidth", "MaxCUHeight", "MaxPartitionDepth", "QuadtreeTULog2MaxSize", "QuadtreeTULog2MinSize", "QuadtreeTUMaxDepthInter", "QuadtreeTUMaxDepthIntra",
            "FastSearch", "SearchRange", "HadamardME", "FEN", "FDM", "QP", "MaxDeltaQP", "MaxCuDQPDepth", "DeltaQpRD", "RDOQ", "RDOQTS", "SAO", "AMP", "TransformSkip", "TransformSkipFast")
    common = "".join(l + "\n" for l in bench.REF_CFG.splitlines() if l.split(":")[0].strip() in keep)
    with tempfile.TemporaryDirectory() as td:
        yuv, cfg = os.path.join(td, "in.yuv"), os.path.join(td, "c.cfg")
        synth.write_yuv(yuv, W, H, BD, 1 + args.steps, 1234)
        open(cfg, "w").write(common + bench.REF_CFG_INTER["ldp_p"][2] + "BipredSearchRange : 4\nInternalBitDepth : 8\nProfile : main\n")
        for arg in (int(v) for v in args.args.split(",")):
            opts = ["--SliceMode=1", f"--SliceArgument={arg}"] if arg else []
            times = []
            for frames in (1, 1 + args.steps):
                out = subprocess.run([enc_bin, "-c", cfg, "-i", yuv, "-wdt", str(W), "-hgt", str(H), "-fr", "50", "-f", str(frames), f"--InputBitDepth={BD}", "-q", str(QP),
                                      "--WaveFrontSynchro=0", "-b", os.path.join(td, "o.bin"), "-o", os.path.join(td, "r.yuv")] + opts,
                                     stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.decode()
                times.append([float(l.split()[2]) for l in out.splitlines() if "Total Time" in l][0])
            run = {"workload": WORKLOAD, "label": "reference encoder, one host core", "hm355_build_id": build_id, "slice_argument": arg, "slices": len(partition(arg)[0]),
                   "ctu_per_s": W_CTU * H_CTU * args.steps / max(1e-9, times[1] - times[0]),
                   "sample": f"the first {args.steps} P pictures of the same stream (HM 'Total Time' of 1 + n pictures minus the I picture alone)"}
            print(json.dumps(run), flush=True)
            append_runs(args.out, [run])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--args", default="0,120,30", help="SliceArgument of the one-stream runs (0: one slice)")
    ap.add_argument("--steps", type=int, default=2, help="P pictures of the one-stream run")
    ap.add_argument("--streams", type=int, default=0, help="also: this many streams in one launch")
    ap.add_argument("--stream-args", default="0,30")
    ap.add_argument("--cpu-reference", action="store_true")
    ap.add_argument("--out", default=os.path.join(_paths.ROOT, "profiles", "slices_timing.json"))
    args = ap.parse_args()
    build_id = hm355.load_library().hm355_build_id().decode()
    if args.cpu_reference:
        cpu_reference(args, build_id)
        return
    if args.args:
        one_stream(args, build_id)
    if args.streams:
        many_streams(args, build_id)


if __name__ == "__main__":
    main()
