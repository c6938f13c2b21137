"""The bit count and estimator state of a 2Nx2N intra CU taken from the luma and chroma counts of its search (cu_bits_from_passes,
hm355_core.h) against the recount of the CU's syntax they replace: the host twin built with -DHM355_CHECK_CU_BITS computes both for every
such CU and reports any that differ in the Q15 count or in one context."""
import re
import subprocess

import numpy as np
import pytest

import common

# A CU recounts its chroma syntax only when it is larger than 8x8 (split transform tree, both chroma cbfs set: the table in hm355_types.h).
# A whole CTU evaluates 1 + 4 + 16 such CUs among its 85 2Nx2N evaluations, a CTU cut by the picture edge fewer of the large ones, so no
# input can exceed 21 / 85 unless CUs fall back that the table does not name.  The whole recount is left to NxN CUs, P / B slices and
# cu_qp_delta: none of the 2Nx2N evaluations of these I-slice inputs is one.
CHROMA_RECOUNT_CAP = 21 / 85
RECOUNT_CAP = 0.0

TWINS = ((), "hostsim_chk"), (("-DHM355_HOSTSIM_REVERSE",), "hostsim_chk_rev")


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("cu_bits")
    return [common.build_hostsim(d, "hostsim", "-DHM355_CHECK_CU_BITS", *flags, exe=exe) for flags, exe in TWINS]


def _run(exe, yuv, w, h, bd, frames, qp, wpp, dump):
    r = subprocess.run([str(exe), str(yuv), str(w), str(h), str(bd), str(frames), str(qp), str(wpp), str(dump)], capture_output=True, text=True)
    s = re.search(r"CU_BITS merged (\d+) chroma_recount (\d+) recount (\d+) mismatch (\d+)", r.stderr)
    assert s, f"no summary line from the cross-check build:\n{r.stderr[-2000:]}"
    merged, chroma, recount, bad = (int(v) for v in s.groups())
    what = f"{exe.name} {w}x{h} qp{qp} wpp{wpp}"
    print(f"{what}: merged {merged}, chroma recount {chroma}, recount {recount}, mismatches {bad}")
    assert bad == 0 and r.returncode == 0, f"{what}: CUs whose bits from the passes differ from the recount:\n{r.stderr[-4000:]}"
    n = merged + chroma + recount
    assert n > 0 and merged > 0
    assert recount <= RECOUNT_CAP * n, f"{what}: {recount} of {n} 2Nx2N evaluations took the whole recount"
    assert chroma <= CHROMA_RECOUNT_CAP * n, f"{what}: {chroma} of {n} 2Nx2N evaluations recounted their chroma syntax"


@pytest.mark.parametrize("name", ["small_128x128_10b_qp37", "wpp_416x240_10b_qp32", "c1_416x240_8b_qp32"])
def test_cu_bits_from_passes_equal_the_recount_on_the_fixture_clips(tmp_path, twins, name):
    """The three I-slice fixture clips, forwards and with the lane loops reversed; the twin's result is still the fixture's."""
    import gen_golden
    import synth
    cfg, frames = common.load_case(name)
    yuv = tmp_path / "in.yuv"
    synth.write_yuv(str(yuv), cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["seed"])
    for exe in twins:
        dump = tmp_path / (exe.name + ".bin")
        _run(exe, yuv, cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["qp"], cfg["wpp"], dump)
        got = gen_golden.parse_dump(str(dump))
        for i, (ctus, rec) in enumerate(frames):
            common.assert_ctus_equal(got[i][0], ctus, f"{exe.name} frame {i}", (cfg["width"], cfg["height"]))
            assert np.array_equal(got[i][1], rec)


@pytest.mark.parametrize("w,h,bd,qp,seed", [(192, 128, 10, 12, 31), (200, 136, 8, 47, 32), (320, 192, 10, 32, 33)])
def test_cu_bits_from_passes_equal_the_recount_on_fresh_inputs(tmp_path, twins, w, h, bd, qp, seed):
    """Fresh inputs at both ends of the QP range and in the middle, two with ragged edges, with and without WPP: split luma trees and dense
    chroma at the low QP, CUs without any coded block at the high one."""
    import synth
    yuv = tmp_path / "in.yuv"
    synth.write_yuv(str(yuv), w, h, bd, 1, seed)
    for exe in twins:
        for wpp in (0, 1):
            _run(exe, yuv, w, h, bd, 1, qp, wpp, tmp_path / f"{exe.name}_{wpp}.bin")
