"""Diagnostic: cost of the LCU-level rate control loop on the device.

  python tools/lcu_rc_timing.py [--streams 32] [--loop-ctus 60] [--out file.json]

1080p 8-bit low-delay P pictures (WaveFrontSynchro on) with seeded synthetic lambda / QP per CTU: the per-CTU loop (hm355_set_ctu_rc,
hm355_run_ctus of one CTU, hm355_ctu_rc_feedback) over the first --loop-ctus CTUs (two CTU rows by default) against the same slice searched
whole (hm355_run_ctus over every CTU), for one stream and
for `--streams` streams in as many slots (one launch per CTU address); then hm355_intra_cost on one 3840x2160 10-bit picture and over the
slots called in turn (kernel time from HIP events, luma bytes read over kernel time).  Prints each phase as it ends, then one JSON line."""
import argparse
import ctypes as C
import json
import time

import numpy as np

import _paths
import hm355
import synth


def p_slice(qp):
    return hm355.inter_slice_params("P", qp, 0.4624 * 2.0 ** ((qp - 12) / 3.0), 1, (1, 0), np.zeros((2, 16), np.int32))


def p_streams(n, w=1920, h=1080, qp=32, seed=5):
    """an encoder with n slots, each holding an open P slice (picture 1 of its stream) that references its own finished I picture"""
    enc = hm355.Encoder(w, h, 8, 1, max_batch=n)
    for s in range(n):
        enc.upload(s, synth.frame(w, h, 8, 0, seed + s))
    enc.run(n, qp - 1)
    enc.deblock_run([(2, qp - 1, np.zeros((2, 16), np.int32))] * n)
    refs = [enc.ref_from_slot(s, 0, False) for s in range(n)]
    sp = p_slice(qp)
    rng = np.random.default_rng(seed)
    qps = (qp + rng.integers(-3, 4, enc.num_ctus)).astype(np.int8)
    lams = sp["lambda"] * 2.0 ** ((qps.astype(np.float64) - qp) / 3.0) * rng.uniform(0.9, 1.1, enc.num_ctus)

    def begin():
        for s in range(n):
            enc.upload(s, synth.frame(w, h, 8, 1, seed + s))
            enc.set_dqp(s, None, 0)
            enc.slice_begin_inter(s, sp, {0: refs[s]})
    return enc, refs, begin, qps, lams


def loop_rate(n, loop_ctus):
    enc, refs, begin, qps, lams = p_streams(n)
    nc = enc.num_ctus
    nl = min(loop_ctus, nc)
    begin()
    t0 = time.perf_counter()
    for a in range(nl):
        for s in range(n):
            enc.set_ctu_rc(s, a, qps[a:a + 1], lams[a:a + 1])
        enc.run_ctus(0, n, a, 1)
        for s in range(n):
            enc.ctu_rc_feedback(s, a, 1)
    t_loop = time.perf_counter() - t0
    for s in range(n):
        enc.slice_end(s)
    begin()
    for s in range(n):
        enc.set_ctu_rc(s, 0, qps, lams)
    t0 = time.perf_counter()
    enc.run_ctus(0, n, 0, nc)
    t_whole = time.perf_counter() - t0
    for s in range(n):
        enc.slice_end(s)
    for r in refs:
        enc.ref_release(r)
    enc.close()
    res = {"streams": n, "ctus_per_picture": nc, "loop_ctus": nl, "loop_s": round(t_loop, 3), "loop_ctu_per_s": round(n * nl / t_loop, 1),
           "whole_s": round(t_whole, 3), "whole_ctu_per_s": round(n * nc / t_whole, 1)}
    print(json.dumps(res), flush=True)
    return res


def intra_cost_rate(slots):
    w, h = 3840, 2160
    enc = hm355.Encoder(w, h, 10, 1, max_batch=slots)
    rng = np.random.default_rng(9)
    planes = [rng.integers(0, 1024, (h, w)).astype(np.uint16), rng.integers(0, 1024, (h // 2, w // 2)).astype(np.uint16),
              rng.integers(0, 1024, (h // 2, w // 2)).astype(np.uint16)]
    for s in range(slots):
        enc.upload(s, planes)
    enc.intra_cost(0)                      # first launch (code object load) not timed
    ms = []
    for s in range(slots):
        enc.intra_cost(s)
        k, _ = kernel_info(enc)
        ms.append(k)
    enc.close()
    luma = w * h * 2
    res = {"picture": "3840x2160 10-bit", "one_ms": round(ms[0], 4), "slots": slots, "mean_ms": round(float(np.mean(ms)), 4),
           "luma_GB_per_s": round(luma / (float(np.mean(ms)) * 1e-3) / 1e9, 1)}
    print(json.dumps(res), flush=True)
    return res


def kernel_info(enc):
    ms, launches = C.c_double(), C.c_int()
    enc.lib.hm355_last_run_info(enc.h_, C.byref(ms), C.byref(launches))
    return ms.value, launches.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--loop-ctus", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = hm355.load_library()
    lib.hm355_build_id.restype = C.c_char_p
    res = {"build_id": lib.hm355_build_id().decode()}
    print(json.dumps(res), flush=True)
    res["intra_cost"] = intra_cost_rate(a.streams)
    res["one_stream"] = loop_rate(1, a.loop_ctus)
    res["many_streams"] = loop_rate(a.streams, a.loop_ctus)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
