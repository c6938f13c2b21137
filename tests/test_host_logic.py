"""CPU suite: host-side logic of the product (schedule, ABI surface, library exports)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import common

ROOT = common.ROOT


def test_library_exports_every_declared_symbol():
    """libhm355.so must load without a GPU and export every function include/hm355.h declares"""
    import hm355
    hdr = open(os.path.join(ROOT, "include", "hm355.h")).read()
    declared = sorted(set(re.findall(r"\b(hm355_[a-z_0-9]+)\s*\(", hdr)))
    assert declared, "no declarations found"
    lib = ctypes.CDLL(hm355.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} is declared in include/hm355.h but not exported"
    assert set(hm355.EXPORTS) == set(declared)


def test_create_rejects_bad_config_and_missing_gpu():
    """argument errors are reported as HM355_ERR_ARG; without a device create() must fail (no CPU fallback)"""
    import hm355
    lib = hm355.load_library()
    h = ctypes.c_void_p()
    bad = hm355.SeqCfg(417, 240, 8, 64, 4, 5, 2, 3, 0, 1)
    assert lib.hm355_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    bad = hm355.SeqCfg(416, 240, 9, 64, 4, 5, 2, 3, 0, 1)
    assert lib.hm355_create(ctypes.byref(bad), ctypes.byref(h)) == -1
    import torch
    if not torch.cuda.is_available():
        ok = hm355.SeqCfg(416, 240, 8, 64, 4, 5, 2, 3, 0, 1)
        rc = lib.hm355_create(ctypes.byref(ok), ctypes.byref(h))
        assert rc == -2, "hm355_create must fail with HM355_ERR_NO_DEVICE when there is no GPU"


def _schedule(wc, hc, wpp, frames, carry=0):
    """python mirror of hm355_build_schedule (hm355_host_common.h) for property checks"""
    def step(x, y):
        if not wpp:
            return y * wc + x
        if carry and hc > 1 and wc > 1 and y == hc - 1:
            return (wc - 1) + 2 * (hc - 2) + 1 + x
        return x + 2 * y
    out = [[] for _ in range(step(wc - 1, hc - 1) + 1)]
    for f in range(frames):
        for y in range(hc):
            for x in range(wc):
                out[step(x, y)].append((f, x, y))
    return out


@pytest.mark.parametrize("wc,hc,wpp,carry", [(7, 4, 1, 0), (7, 4, 0, 0), (60, 34, 1, 0), (1, 3, 1, 0), (2, 2, 1, 0), (7, 4, 1, 1), (30, 17, 1, 1),
                                             (1, 3, 1, 1), (2, 2, 1, 1)])
def test_schedule_respects_dependencies(wc, hc, wpp, carry):
    sched = _schedule(wc, hc, wpp, 2, carry)
    done = {}
    for s, items in enumerate(sched):
        for (f, x, y) in items:
            deps = [(x - 1, y), (x, y - 1), (x - 1, y - 1), (x + 1, y - 1)]
            if not wpp and (x, y) != (0, 0):
                px, py = (x - 1, y) if x > 0 else (wc - 1, y - 1)
                deps.append((px, py))
            if wpp and x == 0 and y > 0 and wc > 1:
                deps.append((1, y - 1))
            if carry and x == 0 and y == hc - 1 and y > 0:      # P slice, last CTU row cut by the picture edge
                deps.append((wc - 1, y - 1))
            for (dx, dy) in deps:
                if 0 <= dx < wc and 0 <= dy < hc:
                    assert done.get((f, dx, dy), 10 ** 9) < s, f"CTU {(x, y)} scheduled before {(dx, dy)}"
        for it in items:
            done[it] = s
    assert len(done) == 2 * wc * hc


@pytest.mark.parametrize("name", ["small_128x128_10b_qp37", "wpp_416x240_10b_qp32", "c1_416x240_8b_qp32"])
def test_hostsim_of_kernel_source_matches_reference_fixture(tmp_path, name):
    """The kernel source (hm355_core.h) compiled for the host with one lane, forwards and with every
    lane-parallel loop reversed, reproduces the reference fixture (the two 416x240 ones hold transform trees of
    depth 2, the small one stops at depth 1).  Debugging aid: the GPU tests are the gate."""
    import synth
    cfg, frames = common.load_case(name)
    yuv = tmp_path / "in.yuv"
    synth.write_yuv(str(yuv), cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["seed"])
    import gen_golden
    for flags, exe in ((), "hostsim"), (("-DHM355_HOSTSIM_REVERSE",), "hostsim_rev"):
        out = common.build_hostsim(tmp_path, "hostsim", *flags, exe=exe)
        dump = tmp_path / (exe + ".bin")
        subprocess.run([str(out), str(yuv), str(cfg["width"]), str(cfg["height"]), str(cfg["bit_depth"]), str(cfg["frames"]),
                        str(cfg["qp"]), str(cfg["wpp"]), str(dump)], check=True)
        got = gen_golden.parse_dump(str(dump))
        for i, (ctus, rec) in enumerate(frames):
            common.assert_ctus_equal(got[i][0], ctus, f"{exe} frame {i}", (cfg["width"], cfg["height"]))
            assert np.array_equal(got[i][1], rec)


def test_hostsim_result_does_not_depend_on_what_the_buffers_held(tmp_path):
    """Everything the search writes before it reads may hold anything: the host twin with its workspace, LDS state, reconstruction planes, decision /
    coefficient / statistics arrays and CABAC hand-off states filled with noise (HM355_DIRTY, three seeds) gives the result of the zero-filled run."""
    import filecmp
    import synth
    out = common.build_hostsim(tmp_path, "hostsim")
    for (w, h, bd, qp, wpp, seed) in [(192, 128, 10, 30, 1, 31), (200, 136, 8, 22, 0, 9)]:
        yuv = tmp_path / f"in_{w}.yuv"
        synth.write_yuv(str(yuv), w, h, bd, 2, seed)
        dumps = []
        for d in (None, "1", "2", "3"):
            dump = tmp_path / f"d_{w}_{d}.bin"
            env = dict(os.environ)
            if d:
                env["HM355_DIRTY"] = d
            subprocess.run([str(out), str(yuv), str(w), str(h), str(bd), "2", str(qp), str(wpp), str(dump)], check=True, env=env)
            dumps.append(str(dump))
        assert all(filecmp.cmp(dumps[0], x, shallow=False) for x in dumps[1:]), f"{w}x{h}: the result depends on uninitialised memory"


def test_hostsim_of_kernel_source_matches_oracle_at_extreme_qps(tmp_path):
    """Dense 32x32 blocks (low QP: RDOQ with every coefficient group coded, sign-bit hiding everywhere), nearly empty ones (high QP),
    with and without WPP: the code paths behind the early terminations of the CU / residual quadtrees and the LDS-resident RDOQ state
    of 32x32 blocks, against the oracle on fresh inputs."""
    import synth, gen_golden, oracle
    out = common.build_hostsim(tmp_path, "hostsim")
    for (w, h, bd, qp, wpp, seed) in [(320, 192, 10, 12, 1, 21), (256, 136, 8, 47, 0, 22), (384, 192, 10, 22, 1, 23), (200, 192, 8, 3, 0, 24)]:
        yuv = tmp_path / f"in{seed}.yuv"
        synth.write_yuv(str(yuv), w, h, bd, 1, seed)
        want_rec, want_ctus = oracle.compress(synth.frame(w, h, bd, 0, seed), bd, qp, wpp)
        dump = tmp_path / f"out{seed}.bin"
        subprocess.run([str(out), str(yuv), str(w), str(h), str(bd), "1", str(qp), str(wpp), str(dump)], check=True)
        got = gen_golden.parse_dump(str(dump))
        common.assert_ctus_equal(got[0][0], want_ctus, f"{w}x{h} qp{qp}", (w, h))
        common.assert_rec_equal(want_rec, got[0][1], w, h, f"{w}x{h} qp{qp}")


HOSTSIM_EDGE_CASES = [n for n in common.EDGE_CASES if n.endswith(("_qp0", "_qp2", "_qp51", "_mrg2_notmvp"))]     # about 25 s each, mostly compilation


@pytest.mark.parametrize("name", common.LDP_CASES[1:] + common.B_CASES + common.LDP_LONG_CASES + HOSTSIM_EDGE_CASES)
def test_hostsim_of_kernel_source_matches_reference_p_slices(tmp_path, name):
    """The P-slice part of the kernel source (hm355_inter.h / hm355_inter_cu.h) compiled for the host with one lane, forwards and
    with every lane-parallel loop reversed: self-checking replay of the reference's HMD2 record stream (rebuilt from the fixture),
    the search of every inter slice and the bitstream pass of every picture."""
    import synth
    import hmd2
    recs = []
    cfg, _, _ = common.load_ldp_case(name, recs)
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump2.bin"
    synth.write_yuv(str(yuv), cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["seed"])
    hmd2.write(str(dump), recs, bits=True)
    for flags, exe in ((), "hostsim_inter"), (("-DHM355_HOSTSIM_REVERSE",), "hostsim_inter_rev"):
        out = common.build_hostsim(tmp_path, "hostsim_inter", *flags, exe=exe)
        r = subprocess.run([str(out), str(yuv), str(dump), str(cfg["width"]), str(cfg["height"]), str(cfg["bit_depth"]), str(cfg["wpp"])],
                           capture_output=True, text=True)
        assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:]
        assert r.stdout.count("bitstream: ok") == cfg["frames"], r.stdout[-2000:]     # the bitstream pass (hm355_bits_kernel.h) of every picture, I slice included


PLAN_IN = ("wc", "hc", "wpp", "max_batch", "n", "ctu0", "ctu1", "inter", "fast", "env_team", "env_team_waves", "share", "team_cap")
PLAN_OUT = ("wsCount", "parallel", "total", "fewWaves", "teamWanted", "waves", "want", "useTeam", "teams", "grid", "groups")
PLAN_COUNTS = [1, 2, 3, 32, 33, 79, 80, 96, 97, 512, 513, 1024, 1279, 1280]


def _plans(exe, rows):
    """hostsim_plan over `rows` (N x 13 integers in the order of PLAN_IN) -> (dict of input columns, dict of output columns)"""
    a = np.ascontiguousarray(rows, np.int32)
    r = subprocess.run([str(exe), "-"], input=a.tobytes(), capture_output=True, check=True)
    o = np.frombuffer(r.stdout, np.int32).reshape(-1, len(PLAN_OUT)).astype(np.int64)
    assert len(o) == len(a)
    a = a.astype(np.int64)
    return {k: a[:, i] for i, k in enumerate(PLAN_IN)}, {k: o[:, i] for i, k in enumerate(PLAN_OUT)}


def test_launch_plan_always_has_a_workgroup_and_a_workspace_per_wavefront(tmp_path):
    """hm355_plan_launch (hm355_host_common.h: what run_begin launches and lane_init allocates) over pictures of 1x1 .. 60x34 CTUs, with and
    without WaveFrontSynchro, max_batch and n on both sides of every threshold, I and P / B launches, fast decisions, HM355_TEAM / HM355_TEAM_WAVES,
    lane shares 1..4, with the team windows there and without: every launch has a workgroup, every wavefront that can take a ticket has a
    workspace, no team searches a P / B slice with a fast-decision switch on, and the thresholds are where the comments of the function put them."""
    exe = common.build_hostsim(tmp_path, "hostsim_plan")
    # every size up to 4x4 CTUs (where numCtus * max_batch * 9 workspaces can be fewer than a workgroup's 12), then strips, the clips of the GPU
    # suite and the bench's 1080p / 4K
    sizes = [(w, h) for w in range(1, 5) for h in range(1, 5)] + [(60, 1), (1, 34), (2, 34), (7, 4), (5, 4), (13, 7), (30, 17), (60, 34)]
    pairs = [(mb, n) for mb in PLAN_COUNTS for n in PLAN_COUNTS if n <= mb]
    BIG = 1 << 20
    def product(*axes):
        """rows of the Cartesian product of `axes` (each a list of tuples), as one int32 array"""
        axes = [np.array(a, np.int32).reshape(len(a), -1) for a in axes]
        idx = np.indices([len(a) for a in axes]).reshape(len(axes), -1)
        return np.concatenate([a[k] for a, k in zip(axes, idx)], axis=1)
    col = lambda *v: [(x,) for x in v]
    # columns: (wc, hc), wpp, (max_batch, n), inter, fast, env_team, env_team_waves, share, team_cap -- whole pictures
    full = np.concatenate([product(sizes, col(0, 1), pairs, col(0, 1), col(0, 1, 7), col(-1, 0, 1), col(0, 5), col(1, 2, 3, 4), col(BIG)),
                           product(sizes, col(0, 1), pairs, col(0, 1), col(0, 1, 7), col(-1, 0, 1), col(0, 5), col(1), col(0))])
    # CTU ranges of hm355_run_rows / hm355_run_ctus: the first CTU, the last one, the first row, the last row
    bands = []
    for k, (w, h) in enumerate(sizes):
        part = product([sizes[k]], col(0, 1), pairs, col(0, 1), col(0, 7), col(-1), col(0), col(1), col(BIG))
        for c0, c1 in sorted({(0, 0), (w * h - 1, w * h - 1), (0, w - 1), ((h - 1) * w, w * h - 1)}):
            bands.append(np.insert(part, 5, [[c0], [c1]], axis=1))
    last = (full[:, 0] * full[:, 1] - 1)[:, None]
    rows = np.concatenate([np.concatenate([full[:, :5], np.zeros_like(last), last, full[:, 5:]], axis=1)] + bands)
    assert rows.shape[1] == len(PLAN_IN)
    i, o = _plans(exe, rows)
    def bad(mask, what):
        k = np.nonzero(mask)[0]
        if len(k):
            j = k[0]
            raise AssertionError(f"{what}: {len(k)} launches, first " + ", ".join(f"{n}={i[n][j]}" for n in PLAN_IN) + " -> " + ", ".join(f"{n}={o[n][j]}" for n in PLAN_OUT))
    team = o["useTeam"] == 1
    assert (o["total"] == i["n"] * (i["ctu1"] - i["ctu0"] + 1)).all() and (o["total"] >= 1).all()
    # at least one workgroup
    bad(np.where(team, o["teams"], o["groups"]) < 1, "a launch without a workgroup")
    # a workspace for every wavefront: workspace index = workgroup * wavefronts per workgroup + wavefront
    bad(~team & (o["groups"] * 12 > o["wsCount"]), "12-search kernel: more wavefronts than workspaces")
    bad(~team & (o["grid"] != o["groups"] * 12), "12-search kernel: grid")
    bad(team & (o["teams"] * o["waves"] > o["wsCount"]), "team kernel: more wavefronts than workspaces")
    bad(team & (o["teams"] > i["team_cap"]), "team kernel: more teams than reconstruction windows")
    bad(team & ((o["teams"] > o["total"]) | (o["teams"] > 512)), "team kernel: more teams than tickets / than 512")
    bad(~team & (o["groups"] * 12 >= o["total"] + 12), "12-search kernel: a workgroup none of whose wavefronts can get a ticket")
    # one workspace per search the device can hold (3,072), fewer for a small batch (nine per CTU: a team), never fewer than a workgroup's 12
    bad(o["wsCount"] != np.maximum(12, np.minimum(3072, i["wc"] * i["hc"] * i["max_batch"] * 9)), "workspaces of a lane")
    # lane share: a launch takes at most its share (5/4 of an equal split of the 3,072 resident searches), rounded up to a workgroup
    cap = 3072 * 5 // (4 * i["share"])
    bad(~team & (i["share"] > 1) & (o["groups"] > (cap + 11) // 12), "12-search kernel: more than the lane's share")
    # fast decisions
    bad(team & (i["inter"] == 1) & (i["fast"] != 0), "a team on a P / B launch with a fast-decision switch on")
    # the thresholds of the comments in hm355_plan_launch
    wpp, n, inter = i["wpp"] == 1, i["n"], i["inter"] == 1
    bad(o["parallel"] != n * np.where(wpp, 16, 1), "parallel")
    bad(o["fewWaves"] != np.where(wpp, n <= 79, n <= 1279), "fewWaves: 1 below 1,280 CTUs at a time (80 WPP pictures), 0 from there on")
    dflt = (i["env_team"] == -1) & (i["team_cap"] > 0)
    want_team = np.where(inter, (i["fast"] == 0) & np.where(wpp, n <= 96, n <= 1024), np.where(wpp, n <= 32, n <= 512))
    bad(dflt & (team != want_team), "team threshold (I: 512 CTUs at a time = 32 WPP pictures; P / B: 96 WPP streams, 1,024 serial ones)")
    bad((i["env_team"] == 0) & team, "HM355_TEAM=0")
    bad((i["env_team"] == 1) & (i["team_cap"] > 0) & (team != ~(inter & (i["fast"] != 0))), "HM355_TEAM=1")
    bad((i["team_cap"] == 0) & team, "a team launch without reconstruction windows")
    bad(team & (o["waves"] != np.where(inter & (i["env_team_waves"] != 5), 9, 5)), "wavefronts per team")
    bad((o["teamWanted"] == 1) & (o["want"] < 1), "teams asked for")
    # the one-CTU picture with max_batch 1 off the team path (P / B slice with a fast-decision switch on, or HM355_TEAM=0)
    one = (i["wc"] * i["hc"] * i["max_batch"] == 1) & ~team
    assert one.any() and (o["groups"][one] == 1).all() and (o["wsCount"][one] == 12).all()
    # the single-launch form prints the same plan
    r = subprocess.run([str(exe)] + [str(v) for v in (7, 4, 1, 120, 120, 0, 27, 0, 0, -1, 0, 1, 0)], capture_output=True, text=True, check=True)
    assert r.stdout.split() == ["wsCount=3072", "parallel=1920", "total=3360", "fewWaves=0", "teamWanted=0", "waves=5", "want=0", "useTeam=0", "teams=0",
                                "grid=3072", "groups=256"]
