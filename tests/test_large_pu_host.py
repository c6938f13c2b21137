"""The closing pass of a 64x64 intra PU taking its 32x32 TUs from the record of the winner's first pass while every earlier one stayed unsplit
(recur_intra_coding_qt, pu64_record_tu / pu64_take_tu, hm355_core.h) in the host twin of the kernel source, plain and with every lane-parallel
loop reversed, against the oracle on fresh synthetic clips: every decision array, cost, coefficient and reconstructed sample must be equal.  The
twin counts the 32x32 TUs of the closing passes taken from the record and those evaluated (HM355_PU64_STATS): on the 128x128 clip 10 and 7 of
the 16 are taken at QP 22 and 32 -- the others follow a TU that kept its split, so both kinds occur -- and all 16 at QP 45.  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import common

CLIPS = {"128x128": (128, 128, 10, 1), "192x128": (192, 128, 8, 11), "256x128": (256, 128, 10, 5)}   # width, height, bit depth, seed of synth.frame
CASES = [("128x128", 22, 1), ("128x128", 32, 1), ("128x128", 45, 1), ("192x128", 32, 1), ("256x128", 22, 1), ("128x128", 32, 0)]   # clip, QP, WPP


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("large_pu")
    return {"plain": common.build_hostsim(d, "hostsim"), "reversed": common.build_hostsim(d, "hostsim", "-DHM355_HOSTSIM_REVERSE", exe="hostsim_rev")}


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    import synth
    d = tmp_path_factory.mktemp("large_pu_clips")
    out = {}
    for name, (w, h, bd, seed) in CLIPS.items():
        planes = synth.frame(w, h, bd, 0, seed)
        path = d / (name + ".yuv")
        with open(path, "wb") as f:
            for p in planes: f.write((p.astype(np.uint8) if bd == 8 else p.astype("<u2")).tobytes())
        out[name] = (planes, str(path))
    return out


_want = {}
def reference(clips, clip, qp, wpp):
    """oracle.compress of a case, computed once and shared by the twins"""
    import oracle
    if (clip, qp, wpp) not in _want: _want[(clip, qp, wpp)] = oracle.compress(clips[clip][0], CLIPS[clip][2], qp, wpp)
    return _want[(clip, qp, wpp)]


def run_twin(exe, clips, clip, qp, wpp, tmp_path):
    """runs the twin; returns its dump and the 32x32 TUs of 64x64 closing passes (taken from the record, evaluated)"""
    import gen_golden
    w, h, bd, _ = CLIPS[clip]
    dump = tmp_path / "out.bin"
    r = subprocess.run([str(exe), clips[clip][1], str(w), str(h), str(bd), "1", str(qp), str(wpp), str(dump)], check=True,
                       env=dict(os.environ, HM355_PU64_STATS="1"), stderr=subprocess.PIPE, text=True)
    c = re.search(r"pu64 closing reused (\d+) evaluated (\d+)", r.stderr)
    assert c, f"no counters of the 64x64 closing passes:\n{r.stderr[-2000:]}"
    return gen_golden.parse_dump(str(dump))[0], tuple(int(v) for v in c.groups())


@pytest.mark.parametrize("which", ["plain", "reversed"])
@pytest.mark.parametrize("clip,qp,wpp", CASES)
def test_twin_equals_oracle(twins, clips, tmp_path, which, clip, qp, wpp):
    w, h, _, _ = CLIPS[clip]
    want_rec, want_ctus = reference(clips, clip, qp, wpp)
    (ctus, rec), (reused, evaluated) = run_twin(twins[which], clips, clip, qp, wpp, tmp_path)
    print(f"{clip} qp{qp} wpp{wpp} {which}: 32x32 TUs of 64x64 closing passes: {reused} from the record, {evaluated} evaluated")
    common.assert_ctus_equal(ctus, want_ctus, f"{clip} qp{qp} wpp{wpp} {which}", (w, h))
    common.assert_rec_equal(want_rec, rec, w, h, "rec")
    n_ctus = (w // 64) * (h // 64)                              # the clips are whole CTUs: one 64x64 PU each, its closing pass has four 32x32 TUs
    assert reused >= n_ctus and reused + evaluated <= 4 * n_ctus, "the first 32x32 TU of every closing pass is taken from the record; a pass has four"
    if clip == "128x128":
        assert (reused, evaluated) == {22: (10, 6), 32: (7, 9), 45: (16, 0)}[qp], "TUs whose earlier siblings all stayed unsplit, and the others"


def test_standalone_twin_under_address_and_undefined_sanitizers(clips, tmp_path):
    """the host twin as a stand-alone program built with -fsanitize=address,undefined (host code only) on the first clip at QP 22: no report, the oracle's decisions, both kinds of TU"""
    exe = common.build_hostsim(tmp_path, "hostsim", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", exe="hostsim_san")
    want_rec, want_ctus = reference(clips, "128x128", 22, 1)
    (ctus, rec), closing = run_twin(exe, clips, "128x128", 22, 1, tmp_path)
    common.assert_ctus_equal(ctus, want_ctus, "sanitized twin", (128, 128))
    common.assert_rec_equal(want_rec, rec, 128, 128, "rec")
    assert closing == (10, 6)
