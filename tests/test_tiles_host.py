"""CPU suite: tiles (hm355_set_tiles).  The fixtures are what they claim; the tile tables and the tile-scan schedule of hm355_host_common.h against
a numpy restatement of TComPicSym::initTiles; the search with tile-restricted neighbours in the kernel source, on the host twin
tests/hostsim/hostsim_tiles.cpp against clips the real reference encoded with tiles (tests/gen_golden_tiles.py)."""
import os
import subprocess

import numpy as np
import pytest

import common

TILE_CASES = ["tiles_ai_2x1_520x136_8b_qp27", "tiles_ai_3x2_776x72_10b_qp32", "tiles_ldp_2x2_512x128_8b_qp30", "tiles_ra_2x2_520x136_10b_qp38"]
INTER_CASES = TILE_CASES[2:]
UNTILED = "ldp_192x128_8b_qp32"
# wCtu, hCtu, column widths, row heights: one tile, the four fixture layouts, 4 x 4 on a 1080p picture, the most columns and rows there can be
LAYOUTS = [(3, 2, (3,), (2,)), (9, 3, (4, 5), (3,)), (13, 2, (4, 4, 5), (1, 1)), (8, 2, (4, 4), (1, 1)), (9, 3, (5, 4), (2, 1)),
           (30, 17, (7, 8, 7, 8), (4, 4, 4, 5)), (80, 22, (4,) * 20, (1,) * 22)]
FIXTURE_LAYOUTS = LAYOUTS[1:5]

DRIVER = r"""
#include "hostsim_common.h"
#include <string>
static std::vector<int> int_list(const char *s) { std::vector<int> v; for (const char *p = s; *p;) { v.push_back(atoi(p)); while (*p && *p != ',') p++; if (*p) p++; } return v; }
int main(int argc, char **argv)
{ // tables <wCtu> <hCtu> <cols> <rows>            -> "ok" + per CTU: tile x0 x1 y0 y1 prev scanPrev rsToTs tsToRs, or "refused: <reason>"
  // uniform <wCtu> <hCtu> <ncols> <nrows>        -> the column widths, then the row heights
  // schedule <wCtu> <hCtu> <wpp> <carry> <frames> <cols|0> <rows|0> <carryTiles> <width> <height>   -> per item: step frame x y
  // plan <wCtu> <hCtu> <maxBatch> <n> <anyInter> <chains>   -> parallel fewWaves teamWanted waves want maxItems
  const std::string cmd = argv[1]; const int wCtu = atoi(argv[2]), hCtu = atoi(argv[3]);
  if (cmd == "uniform") {
    int cw[64], rh[64]; const int nc = atoi(argv[4]), nr = atoi(argv[5]);
    hm355_tile_uniform_spacing(wCtu, hCtu, nc, nr, cw, rh);
    for (int i = 0; i < nc; i++) printf("%d ", cw[i]); printf("\n"); for (int i = 0; i < nr; i++) printf("%d ", rh[i]); printf("\n");
    return 0;
  }
  if (cmd == "tables") {
    const std::vector<int> c = int_list(argv[4]), r = int_list(argv[5]);
    hm355_tile_tables t; t.cols = -7;
    const char *why = hm355_build_tiles(wCtu, hCtu, (int)c.size(), c.data(), (int)r.size(), r.data(), &t);
    if (why) { printf("refused: %s\n", why); return t.cols == -7 ? 0 : 3; }
    printf("ok\n");
    for (int a = 0; a < wCtu * hCtu; a++) printf("%d %d %d %d %d %d %d %d %d\n", t.tileOf[a], t.ctu[a].x0, t.ctu[a].x1, t.ctu[a].y0, t.ctu[a].y1, t.ctu[a].prev, t.ctu[a].scanPrev, t.rsToTs[a], t.tsToRs[a]);
    return 0;
  }
  if (cmd == "schedule") {
    std::vector<WorkItem> items; std::vector<int> start; hm355_tile_tables t; const bool tiled = argv[7][0] != '0';
    if (tiled) { const std::vector<int> c = int_list(argv[7]), r = int_list(argv[8]); if (hm355_build_tiles(wCtu, hCtu, (int)c.size(), c.data(), (int)r.size(), r.data(), &t)) return 3; }
    if (argc > 12 && argv[12][0] == 'd') hm355_build_schedule(wCtu, hCtu, atoi(argv[4]), atoi(argv[6]), items, start, atoi(argv[5]));      // the call as it was before tiles
    else hm355_build_schedule(wCtu, hCtu, atoi(argv[4]), atoi(argv[6]), items, start, atoi(argv[5]), 0, 0, -1, tiled ? &t : NULL, atoi(argv[9]), atoi(argv[10]), atoi(argv[11]));
    for (size_t s = 0; s + 1 < start.size(); s++) for (int i = start[s]; i < start[s + 1]; i++) printf("%d %d %d %d\n", (int)s, items[i].frame, items[i].ctuX, items[i].ctuY);
    return 0;
  }
  if (cmd == "plan") {
    const int maxBatch = atoi(argv[4]), n = atoi(argv[5]), anyInter = atoi(argv[6]), chains = atoi(argv[7]);
    const hm355_launch_plan p = hm355_plan_launch(wCtu, hCtu, 0, maxBatch, n, 0, wCtu * hCtu - 1, anyInter, 0, -1, 0, 1, 1 << 20, chains);
    const hm355_launch_plan q = hm355_plan_launch(wCtu, hCtu, 0, maxBatch, n, 0, wCtu * hCtu - 1, anyInter, 0, -1, 0, 1, 1 << 20);
    printf("%lld %d %d %d %d %d\n", p.parallel, p.fewWaves, p.teamWanted, p.waves, p.want, hm355_max_items_per_step(wCtu, hCtu, 0, n, chains));
    printf("%lld %d %d %d %d %d\n", q.parallel, q.fewWaves, q.teamWanted, q.waves, q.want, hm355_max_items_per_step(wCtu, hCtu, 0, n));
    return 0;
  }
  return 2;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the pure host functions of hm355_host_common.h behind a command line"""
    d = tmp_path_factory.mktemp("tiles_driver")
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
    return ",".join(str(x) for x in v)


def fixture_layout(name):
    g = np.load(os.path.join(common.GOLD, name + ".npz"))
    return tuple(int(v) for v in g["tile_cols"]), tuple(int(v) for v in g["tile_rows"]), int(g["tile_uniform"])


def init_tiles(w_ctu, h_ctu, cols, rows):
    """TComPicSym::initTiles and the address maps restated: per raster address (tile, x0, x1, y0, y1, prev, scan_prev, rs_to_ts), and ts_to_rs"""
    cb = np.concatenate([[0], np.cumsum(cols)]); rb = np.concatenate([[0], np.cumsum(rows)])
    assert cb[-1] == w_ctu and rb[-1] == h_ctu
    order = [(r, c, y, x) for r in range(len(rows)) for c in range(len(cols)) for y in range(rb[r], rb[r + 1]) for x in range(cb[c], cb[c + 1])]
    out = np.zeros((w_ctu * h_ctu, 8), int); ts_to_rs = np.zeros(w_ctu * h_ctu, int)
    last = -1
    for ts, (r, c, y, x) in enumerate(order):
        a = y * w_ctu + x
        first = y == rb[r] and x == cb[c]
        out[a] = (r * len(cols) + c, cb[c], cb[c + 1], rb[r], rb[r + 1], -1 if first else last, last, ts)
        ts_to_rs[ts] = a; last = a
    return out, ts_to_rs


def test_fixtures_are_tiled_and_differ_from_the_untiled_run():
    """every clip: rows x cols substreams in every 'B' record, at least half of the CTUs of every picture differ from the reference's untiled
    run, three inter slices or more in the inter clips, the file below 700,000 bytes"""
    for name in TILE_CASES:
        cols, rows, _ = fixture_layout(name)
        bits = {}
        cfg, slices, _ = common.load_ldp_case(name, bits=bits)
        n = ((cfg["width"] + 63) // 64) * ((cfg["height"] + 63) // 64)
        assert sum(cols) * sum(rows) == n and len(cols) * len(rows) > 1 and cfg["wpp"] == 0
        assert len(bits) == len(slices) and all(len(b["substreams"]) == len(cols) * len(rows) for b in bits.values())
        diff = np.load(os.path.join(common.GOLD, name + ".npz"))["diff_ctus_vs_off"]
        assert len(diff) == len(slices) and all(2 * int(d) >= n for d in diff), f"{name}: {diff}"
        inter = sum(int(r["slice_type"]) != 2 for r in slices)
        assert inter >= 3 if name in INTER_CASES else inter == 0
        assert os.path.getsize(os.path.join(common.GOLD, name + ".npz")) < 700000


def test_uniform_fixture_layouts_follow_the_uniform_formula(driver):
    seen = 0
    for name in TILE_CASES:
        cols, rows, uniform = fixture_layout(name)
        if not uniform:
            continue
        seen += 1
        out = driver("uniform", sum(cols), sum(rows), len(cols), len(rows)).splitlines()
        assert tuple(int(v) for v in out[0].split()) == cols and tuple(int(v) for v in out[1].split()) == rows, name
    assert seen == 2
    out = driver("uniform", 30, 17, 4, 4).splitlines()
    assert out[0].split() == ["7", "8", "7", "8"] and out[1].split() == ["4", "4", "4", "5"]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{len(l[2])}x{len(l[3])}_on_{l[0]}x{l[1]}")
def test_tile_tables_match_init_tiles(driver, layout):
    w_ctu, h_ctu, cols, rows = layout
    out = driver("tables", w_ctu, h_ctu, _csv(cols), _csv(rows)).splitlines()
    assert out[0] == "ok"
    got = np.array([[int(v) for v in line.split()] for line in out[1:]])
    want, ts_to_rs = init_tiles(w_ctu, h_ctu, cols, rows)
    assert np.array_equal(got[:, :8], want) and np.array_equal(got[:, 8], ts_to_rs)
    n = w_ctu * h_ctu
    assert sorted(got[:, 7]) == list(range(n)) and np.array_equal(got[got[:, 7], 8], np.arange(n)) and np.array_equal(got[got[:, 8], 7], np.arange(n))
    starts = [a for a in range(n) if a % w_ctu == got[a, 1] and a // w_ctu == got[a, 3]]
    assert len(starts) == len(cols) * len(rows) and all(got[a, 5] == -1 for a in starts)
    assert all(got[a, 5] == got[a, 6] >= 0 for a in range(n) if a not in starts)
    assert sum(got[a, 6] == -1 for a in range(n)) == 1 and got[0, 6] == -1


@pytest.mark.parametrize("args, reason", [
    ((9, 3, "3,6", "3"), "narrower than 4 CTUs"), ((9, 3, "4,4", "3"), "column widths do not sum"), ((9, 3, "4,5", "2"), "row heights do not sum"),
    ((9, 3, "4,5", "3,0"), "lower than 1 CTU"), ((84, 2, _csv((4,) * 21), "2"), "more than 20"), ((4, 23, "4", _csv((1,) * 23)), "more than 20"),
    ((9, 3, "4,6", "3"), "column widths do not sum")])
def test_tile_layouts_that_are_refused(driver, args, reason):
    """... and a refused layout leaves the caller's tables untouched (the driver returns 3 otherwise)"""
    out = driver("tables", *args)
    assert out.startswith("refused: ") and reason in out, out


def _schedule(driver, *args):
    return [tuple(int(v) for v in line.split()) for line in driver("schedule", *args).splitlines()]


@pytest.mark.parametrize("layout", FIXTURE_LAYOUTS, ids=lambda l: f"{len(l[2])}x{len(l[3])}_on_{l[0]}x{l[1]}")
def test_schedule_orders_every_ctu_behind_its_predecessor(driver, layout):
    w_ctu, h_ctu, cols, rows = layout
    want, _ = init_tiles(w_ctu, h_ctu, cols, rows)
    for carry_tiles in (0, 1):
        items = _schedule(driver, w_ctu, h_ctu, 0, 0, 2, _csv(cols), _csv(rows), carry_tiles, w_ctu * 64 - 56, h_ctu * 64 - 56)
        step = {(f, y * w_ctu + x): s for s, f, x, y in items}
        assert len(step) == len(items) == 2 * w_ctu * h_ctu
        for (f, a), s in step.items():
            if want[a, 5] >= 0:
                assert step[(f, want[a, 5])] < s
            else:
                assert s == 0 or carry_tiles
        widest = max(sum(1 for it in items if it[0] == s) for s in set(it[0] for it in items))
        assert widest == 2 * len(cols) * len(rows) or (carry_tiles and len(rows) > 1)


def test_schedule_with_one_tile_is_the_untiled_schedule(driver):
    for w_ctu in range(1, 10):
        for h_ctu in range(1, 4):
            for wpp in (0, 1):
                for carry in (0, 1):
                    before = _schedule(driver, w_ctu, h_ctu, wpp, carry, 2, "0", "0", 0, 0, 0, "d")
                    assert before == _schedule(driver, w_ctu, h_ctu, wpp, carry, 2, "0", "0", 1, w_ctu * 64 - 8, h_ctu * 64 - 8)
                    assert before == _schedule(driver, w_ctu, h_ctu, wpp, carry, 2, str(w_ctu), str(h_ctu), 1, w_ctu * 64 - 8, h_ctu * 64 - 8)
                    if not wpp:
                        assert [s for s, f, _, _ in before if f == 0] == list(range(w_ctu * h_ctu))


def test_ra_layout_carries_the_integer_mvs_into_the_bottom_tiles(driver):
    """520x136 with tiles (5, 4) x (2, 1): the bottom tile row is one CTU high and cut by the picture edge, so in a P / B slice the first CTU of
    each bottom tile is ordered behind the last CTU of the tile before it in tile scan; an I slice has no such dependency"""
    w_ctu, h_ctu, cols, rows = FIXTURE_LAYOUTS[3]
    want, ts_to_rs = init_tiles(w_ctu, h_ctu, cols, rows)
    for inter in (0, 1):
        step = {y * w_ctu + x: s for s, f, x, y in _schedule(driver, w_ctu, h_ctu, 0, 0, 1, _csv(cols), _csv(rows), inter, 520, 136)}
        for first in (18, 23):                                    # the first CTUs of the two bottom tiles
            assert want[first, 5] == -1 and want[first, 6] >= 0
            assert (step[first] > step[want[first, 6]]) if inter else step[first] == 0
        assert step[5] == 0                                       # the second tile of the top row starts at once either way
    # the same layout on a picture of whole CTUs: nothing is carried
    step = {y * w_ctu + x: s for s, f, x, y in _schedule(driver, w_ctu, h_ctu, 0, 0, 1, _csv(cols), _csv(rows), 1, 576, 192)}
    assert step[18] == step[23] == 0


def test_launch_plan_counts_the_tiles_as_chains(driver):
    """80 pictures of 2 tiles offer 160 CTUs at a time; without tiles the plan is what it was"""
    with_tiles, without = [[int(v) for v in line.split()] for line in driver("plan", 9, 3, 80, 80, 0, 2).splitlines()]
    assert with_tiles[0] == 160 and with_tiles[5] == 160 and with_tiles[2] == 1 and with_tiles[4] == 162
    assert without[0] == 80 and without[5] == 80 and without[4] == 82
    one, _ = [[int(v) for v in line.split()] for line in driver("plan", 30, 17, 1, 1, 1, 16).splitlines()]
    assert one[0] == 16 and one[4] == 18


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
    d = tmp_path_factory.mktemp("hostsim_tiles")
    return {"fwd": common.build_hostsim(d, "hostsim_tiles"), "rev": common.build_hostsim(d, "hostsim_tiles", "-DHM355_HOSTSIM_REVERSE", exe="hostsim_tiles_rev")}


@pytest.mark.parametrize("name", TILE_CASES)
def test_hostsim_tiles_matches_reference(tmp_path, twins, name):
    """the kernel source on the host with one lane, forwards and with every lane-parallel loop reversed, with the fixture's tile layout: every
    slice bit for bit (decisions, motion, coefficients, costs, reconstruction)"""
    n, args = _replay_inputs(tmp_path, name)
    cols, rows, _ = fixture_layout(name)
    for exe in twins.values():
        r = subprocess.run([str(exe)] + args + [_csv(cols), _csv(rows)], capture_output=True, text=True)
        assert r.returncode == 0 and "all bit-exact" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
        assert f"{n} slices, {len(cols) * len(rows)} tiles" in r.stdout


@pytest.mark.parametrize("name", ["tiles_ai_2x1_520x136_8b_qp27", "tiles_ldp_2x2_512x128_8b_qp30"])
def test_hostsim_without_tiles_does_not_reproduce_the_clip(tmp_path, twins, name):
    _, args = _replay_inputs(tmp_path, name)
    r = subprocess.run([str(twins["fwd"])] + args + ["0", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "MISMATCH" in r.stdout, "the fixture should not be reproduced without tiles"


def test_hostsim_without_tiles_is_the_untiled_search(tmp_path, twins):
    n, args = _replay_inputs(tmp_path, UNTILED)
    r = subprocess.run([str(twins["fwd"])] + args + ["0", "0"], capture_output=True, text=True)
    assert r.returncode == 0 and f"{n} slices, 1 tiles, all bit-exact" in r.stdout, r.stdout[-2000:]
