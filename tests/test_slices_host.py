"""CPU suite: slices (hm355_set_slices).  The fixtures are what they claim; hm355_fixed_ctu_slices, the refused partitions and the per-slice schedule
of hm355_host_common.h against a numpy restatement of the reference's SliceMode=1 rule; the search with slice-restricted neighbours in the kernel
source, on the host twin tests/hostsim/hostsim_slices.cpp against clips the real reference encoded with slices (tests/gen_golden_slices.py)."""
import os
import subprocess

import numpy as np
import pytest

import common
from slices_common import INTER_CASES, MAX_BYTES, SLICE_CASES, fixed_ctu_slices, load_slices_case, slice_of

UNSLICED = "ldp_192x128_8b_qp32"
# wCtu, hCtu, WaveFrontSynchro, SliceArgument: the three fixtures, the WaveFrontSynchro clip of the generator, one slice per row of a 1080p picture
PARTITIONS = [(6, 4, 0, 8), (6, 3, 0, 4), (5, 3, 0, 7), (6, 4, 1, 9), (30, 17, 0, 30), (30, 17, 1, 30)]

DRIVER = r"""
#include "hostsim_common.h"
#include <string>
static std::vector<int> int_list(const char *s) { std::vector<int> v; for (const char *p = s; *p;) { v.push_back(atoi(p)); while (*p && *p != ',') p++; if (*p) p++; } return v; }
int main(int argc, char **argv)
{ // fixed <wCtu> <hCtu> <wpp> <arg>                 -> the count, then the first CTUs
  // sweep                                          -> every (w 1..9, h 1..4, arg 1..w*h, wpp 0..1): "w h wpp arg : first CTUs"
  // tables <wCtu> <hCtu> <wpp> <first CTUs>         -> "ok" + per CTU: first end, or "refused: <reason>" (exit 3 when the caller's table was touched)
  // schedule <wCtu> <hCtu> <wpp> <carry> <frames> <first CTUs|-> <carrySlices> <width> <height> [d]   -> per item: step frame x y
  const std::string cmd = argv[1];
  if (cmd == "sweep") {
    for (int w = 1; w <= 9; w++) for (int h = 1; h <= 4; h++) for (int wpp = 0; wpp < 2; wpp++) for (int arg = 1; arg <= w * h; arg++) {
      int f[64]; const int n = hm355_slice_fixed_ctus(w, h, wpp, arg, f, 64);
      printf("%d %d %d %d :", w, h, wpp, arg); for (int i = 0; i < n; i++) printf(" %d", f[i]); printf("\n");
    }
    return 0;
  }
  const int wCtu = atoi(argv[2]), hCtu = atoi(argv[3]);
  if (cmd == "fixed") {
    int f[1024]; const int n = hm355_slice_fixed_ctus(wCtu, hCtu, atoi(argv[4]), atoi(argv[5]), f, 1024);
    printf("%d\n", n); for (int i = 0; i < n; i++) printf("%d ", f[i]); printf("\n");
    return 0;
  }
  if (cmd == "tables") {
    const std::vector<int> f = int_list(argv[5]);
    hm355_slice_tables t; t.first.assign(1, -7);
    const char *why = hm355_build_slices(wCtu, hCtu, atoi(argv[4]), (int)f.size(), f.data(), &t);
    if (why) { printf("refused: %s\n", why); return t.first.size() == 1 && t.first[0] == -7 && t.ctu.empty() ? 0 : 3; }
    printf("ok\n");
    for (int a = 0; a < wCtu * hCtu; a++) printf("%d %d\n", t.ctu[a].first, t.ctu[a].end);
    return 0;
  }
  if (cmd == "schedule") {
    std::vector<WorkItem> items; std::vector<int> start; hm355_slice_tables t; const bool sliced = argv[7][0] != '-';
    if (sliced) { const std::vector<int> f = int_list(argv[7]); if (hm355_build_slices(wCtu, hCtu, 0, (int)f.size(), f.data(), &t)) return 3; }
    if (argc > 11 && argv[11][0] == 'd') hm355_build_schedule(wCtu, hCtu, atoi(argv[4]), atoi(argv[6]), items, start, atoi(argv[5]));      // the call as it was before slices
    else hm355_build_schedule(wCtu, hCtu, atoi(argv[4]), atoi(argv[6]), items, start, atoi(argv[5]), 0, 0, -1, NULL, atoi(argv[8]), atoi(argv[9]), atoi(argv[10]), sliced ? &t : NULL);
    for (size_t s = 0; s + 1 < start.size(); s++) for (int i = start[s]; i < start[s + 1]; i++) printf("%d %d %d %d\n", (int)s, items[i].frame, items[i].ctuX, items[i].ctuY);
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the pure host functions of hm355_host_common.h behind a command line"""
    d = tmp_path_factory.mktemp("slices_driver")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.run(["g++", "-O1", "-std=c++14", "-w", "-I", os.path.join(common.ROOT, "tests", "hostsim"), "-o", str(exe), str(src)], check=True)

    def run(*args):
        r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout
    return run


def _csv(v):
    return ",".join(str(int(x)) for x in v)


def test_fixtures_are_sliced_and_differ_from_the_unsliced_run():
    """every clip: one 'S' record per picture and one 'B' record per slice, the partition the SliceMode=1 rule gives, the first CTU of every slice
    but the first differs from the reference's unsliced run in every picture, two inter pictures or more in the inter clips, below 700,000 bytes"""
    for name in SLICE_CASES:
        cfg, slices, finals, sao, bits, extra = load_slices_case(name)
        w_ctu, h_ctu = (cfg["width"] + 63) // 64, (cfg["height"] + 63) // 64
        first = [int(v) for v in extra["slice_first_ctu"]]
        assert cfg["wpp"] == 0 and len(first) > 1 and first == fixed_ctu_slices(w_ctu, h_ctu, 0, int(extra["slice_arg"]))
        assert len(slices) == cfg["frames"] == len(finals) == len(sao) == len(bits)
        assert len(set(int(r["poc"]) for r in slices)) == len(slices)
        for r in slices:
            b = bits[int(r["poc"])]
            assert len(b) == len(first) and all(sum(len(s) > 0 for s in x["substreams"]) == 1 for x in b)
        diff = extra["diff_first_ctu_vs_off"]
        assert diff.shape == (len(slices), len(first)) and diff[:, 1:].all(), f"{name}: {diff}"
        for r, d in zip(slices, diff):
            assert int(r["slice_type"]) != 2 or d[0] == 0
        inter = sum(int(r["slice_type"]) != 2 for r in slices)
        assert inter >= 2 if name in INTER_CASES else inter == 0
        assert os.path.getsize(os.path.join(common.GOLD, name + ".npz")) < MAX_BYTES


def test_fixed_ctu_slices_match_the_slice_mode_1_rule(driver):
    seen = 0
    for line in driver("sweep").splitlines():
        head, tail = line.split(":")
        w, h, wpp, arg = (int(v) for v in head.split())
        assert [int(v) for v in tail.split()] == fixed_ctu_slices(w, h, wpp, arg), line
        seen += 1
    assert seen == 2 * sum(w * h for w in range(1, 10) for h in range(1, 5))
    for w, h, wpp, arg in PARTITIONS:
        out = driver("fixed", w, h, wpp, arg).splitlines()
        want = fixed_ctu_slices(w, h, wpp, arg)
        assert int(out[0]) == len(want) and [int(v) for v in out[1].split()] == want
    assert fixed_ctu_slices(6, 4, 1, 9) == [0, 9, 12, 21] and fixed_ctu_slices(6, 4, 0, 9) == [0, 9, 18]
    assert fixed_ctu_slices(30, 17, 0, 30) == list(range(0, 510, 30))
    for name in SLICE_CASES:
        cfg, _, _, _, _, extra = load_slices_case(name)
        assert (((cfg["width"] + 63) // 64), ((cfg["height"] + 63) // 64), 0, int(extra["slice_arg"])) in PARTITIONS


@pytest.mark.parametrize("part", PARTITIONS, ids=lambda p: f"{p[0]}x{p[1]}_wpp{p[2]}_arg{p[3]}")
def test_slice_tables(driver, part):
    w, h, wpp, arg = part
    first = fixed_ctu_slices(w, h, wpp, arg)
    out = driver("tables", w, h, wpp, _csv(first)).splitlines()
    assert out[0] == "ok"
    got = np.array([[int(v) for v in line.split()] for line in out[1:]])
    ends = first[1:] + [w * h]
    k = slice_of(first, w * h)
    assert np.array_equal(got[:, 0], np.asarray(first)[k]) and np.array_equal(got[:, 1], np.asarray(ends)[k])


@pytest.mark.parametrize("args, reason", [
    ((6, 4, 0, "1,8"), "does not start at CTU 0"), ((6, 4, 0, "0,8,8"), "not ascending"), ((6, 4, 0, "0,16,8"), "not ascending"),
    ((6, 4, 0, "0,24"), "past the picture"), ((6, 4, 1, "0,9,18"), "must end with that row"), ((6, 4, 1, "0,3"), "must end with that row")])
def test_partitions_that_are_refused(driver, args, reason):
    """... and a refused partition leaves the caller's table untouched (the driver returns 3 otherwise)"""
    out = driver("tables", *args)
    assert out.startswith("refused: ") and reason in out, out


def test_wpp_partitions_that_keep_the_row_rule_are_accepted(driver):
    assert driver("tables", 6, 4, 1, "0,9,12,21").startswith("ok") and driver("tables", 6, 4, 1, "0,6,9,12").startswith("ok")


def _schedule(driver, *args):
    return [tuple(int(v) for v in line.split()) for line in driver("schedule", *args).splitlines()]


@pytest.mark.parametrize("part", [p for p in PARTITIONS if not p[2]], ids=lambda p: f"{p[0]}x{p[1]}_arg{p[3]}")
def test_schedule_orders_every_ctu_behind_its_predecessors(driver, part):
    """a CTU follows the CTU before it in its slice; in a P / B picture a slice whose first CTU the picture edge cuts follows the CTU before it
    (m_integerMv2Nx2N); every other slice start is free.  Two pictures of s slices offer 2 s CTUs in the widest step"""
    w, h, _, arg = part
    first = fixed_ctu_slices(w, h, 0, arg)
    width, height = w * 64 - 56, h * 64 - 56
    for carry in (0, 1):
        items = _schedule(driver, w, h, 0, 0, 2, _csv(first), carry, width, height)
        step = {(f, y * w + x): s for s, f, x, y in items}
        assert len(step) == len(items) == 2 * w * h
        for (f, a), s in step.items():
            cut = a % w == w - 1 or a // w == h - 1
            if a not in first:
                assert step[(f, a - 1)] == s - 1
            elif a and carry and cut:
                assert step[(f, a - 1)] < s
            else:
                assert s == 0
        widest = max(sum(1 for it in items if it[0] == s) for s in set(it[0] for it in items))
        free = sum(1 for a in first if not (a and carry and (a % w == w - 1 or a // w == h - 1)))
        assert widest == 2 * len(first) if not carry else widest >= 2 * min(free, len(first))
        if not carry:
            assert widest == 2 * len(first)


def test_schedule_with_one_slice_is_the_schedule_of_today(driver):
    for w in range(1, 10):
        for h in range(1, 4):
            for wpp in (0, 1):
                for carry in (0, 1):
                    before = _schedule(driver, w, h, wpp, carry, 2, "-", 0, 0, 0, "d")
                    assert before == _schedule(driver, w, h, wpp, carry, 2, "-", 1, w * 64 - 8, h * 64 - 8)
                    assert before == _schedule(driver, w, h, wpp, carry, 2, "0", 1, w * 64 - 8, h * 64 - 8)


def test_fixture_layouts_carry_the_integer_mvs_into_slices_cut_by_the_picture_edge(driver):
    """328x136 with slices every 4 CTUs: CTUs 12 and 16 start slices in the bottom CTU row, which the picture edge cuts; 264x136 every 7: CTU 14
    is the corner CTU.  In a P / B picture they follow the CTU before them, in an I picture they start at once; so do slices the edge does not cut"""
    for (w, h, arg, width, height), carried, free in (((6, 3, 4, 328, 136), (12, 16), (4, 8)), ((5, 3, 7, 264, 136), (14,), (7,))):
        first = fixed_ctu_slices(w, h, 0, arg)
        for inter in (0, 1):
            step = {y * w + x: s for s, f, x, y in _schedule(driver, w, h, 0, 0, 1, _csv(first), inter, width, height)}
            for a in carried:
                assert (step[a] == step[a - 1] + 1) if inter else step[a] == 0
            for a in free:
                assert step[a] == 0
    # a slice that starts at the right edge of a picture whose last CTU column is partial
    step = {y * 3 + x: s for s, f, x, y in _schedule(driver, 3, 2, 0, 0, 1, "0,2", 1, 136, 128)}
    assert step[2] == 2
    step = {y * 3 + x: s for s, f, x, y in _schedule(driver, 3, 2, 0, 0, 1, "0,2", 1, 192, 128)}
    assert step[2] == 0


# ---- the host twin ----
def _replay_inputs(tmp_path, name):
    import hmd2
    import synth
    recs = []
    cfg, slices, _ = common.load_ldp_case(name, recs)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump2.bin"
    synth.write_yuv(str(yuv), w, h, bd, cfg["frames"], cfg["seed"])
    hmd2.write(str(dump), recs)
    return len(slices), [str(yuv), str(dump), str(w), str(h), str(bd)]


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostsim_slices")
    return {"fwd": common.build_hostsim(d, "hostsim_slices"), "rev": common.build_hostsim(d, "hostsim_slices", "-DHM355_HOSTSIM_REVERSE", exe="hostsim_slices_rev")}


@pytest.mark.parametrize("name", SLICE_CASES)
def test_hostsim_slices_matches_reference(tmp_path, twins, name):
    """the kernel source on the host with one lane, forwards and with every lane-parallel loop reversed, with the fixture's partition: every
    picture bit for bit (decisions, motion, coefficients, costs, reconstruction)"""
    n, args = _replay_inputs(tmp_path, name)
    first = load_slices_case(name)[5]["slice_first_ctu"]
    for exe in twins.values():
        r = subprocess.run([str(exe)] + args + [_csv(first)], capture_output=True, text=True)
        assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
        assert f"{n} pictures, {len(first)} slices" in r.stdout


@pytest.mark.parametrize("name", SLICE_CASES[:2])
def test_hostsim_without_the_partition_does_not_reproduce_the_clip(tmp_path, twins, name):
    _, args = _replay_inputs(tmp_path, name)
    r = subprocess.run([str(twins["fwd"])] + args + ["0"], capture_output=True, text=True)
    assert r.returncode == 1 and "MISMATCH" in r.stdout, "the fixture should not be reproduced without its slices"


def test_hostsim_with_one_slice_is_the_search_of_today(tmp_path, twins):
    n, args = _replay_inputs(tmp_path, UNSLICED)
    r = subprocess.run([str(twins["fwd"])] + args + ["0"], capture_output=True, text=True)
    assert r.returncode == 0 and f"{n} pictures, 1 slices, all bit-exact" in r.stdout, r.stdout[-2000:]


def test_one_slice_path_against_the_parent_lies_inside_the_parents_spread():
    """profiles/slices_bench_ab.json, the headline benchmark on the parent's build and on this one: the difference of the mean step times is no
    larger than the distance between the parent's own slowest and fastest timed step; recomputed from the recorded steps"""
    import json
    d = json.load(open(os.path.join(common.ROOT, "profiles", "slices_bench_ab.json")))
    ps, ts = d["parent_timed_step_ms"], d["this_timed_step_ms"]
    assert len(ps) == len(ts) == 20 and d["parent"]["config"]["build_id"] != d["this"]["config"]["build_id"]
    spread = max(ps) - min(ps)
    diff = sum(ts) / len(ts) - sum(ps) / len(ps)
    assert abs(spread - d["parent_spread_ms_slowest_minus_fastest_timed_step"]) < 1e-6 and abs(diff - d["this_minus_parent_ms_per_step"]) < 1e-6
    assert diff <= spread and d["slower_by_more_than_the_parent_spread"] is False
