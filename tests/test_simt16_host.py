"""The candidates-in-lanes first pass of 8x8 and 16x16 intra PUs (simt_luma_first_pass<3> / <4>, hm355_simt.h) in the host twin of the kernel
source, plain and with every lane-parallel loop reversed, against the oracle on fresh synthetic clips: every decision array, cost, coefficient
and reconstructed sample must be equal.  The twin counts the candidates of each first pass and the batches it took, per size
(HM355_S16_STATS): at QP 22 the clips must hold 16x16 PUs with 3, 4 and 5 candidates and -- a 16x16 batch holding four -- PUs that took two
batches, and 8x8 PUs with 8 and with more than 8 candidates, every one of them in exactly one batch.  CPU only."""
import os, re, subprocess
import numpy as np
import pytest
import common

CLIPS = {"128x128": (128, 128, 10, 1), "80x80": (80, 80, 10, 3), "192x128": (192, 128, 8, 11)}   # width, height, bit depth, seed of synth.frame
CASES = [("128x128", 4, 1), ("128x128", 22, 1), ("128x128", 37, 1), ("128x128", 22, 0), ("80x80", 22, 1), ("192x128", 22, 1)]   # clip, QP, WPP


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("simt16")
    return {"plain": common.build_hostsim(d, "hostsim"), "reversed": common.build_hostsim(d, "hostsim", "-DHM355_HOSTSIM_REVERSE", exe="hostsim_rev")}


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    import synth
    d = tmp_path_factory.mktemp("simt16_clips")
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
    """oracle.compress of a case, computed once and shared by both twins"""
    import oracle
    if (clip, qp, wpp) not in _want: _want[(clip, qp, wpp)] = oracle.compress(clips[clip][0], CLIPS[clip][2], qp, wpp)
    return _want[(clip, qp, wpp)]


def run_twin(exe, clips, clip, qp, wpp, tmp_path):
    import gen_golden
    w, h, bd, _ = CLIPS[clip]
    dump = tmp_path / "out.bin"
    r = subprocess.run([str(exe), clips[clip][1], str(w), str(h), str(bd), "1", str(qp), str(wpp), str(dump)], check=True,
                       env=dict(os.environ, HM355_S16_STATS="1"), stderr=subprocess.PIPE, text=True)
    cand, batches, cand8, batches8 = ([int(v) for v in re.search(name + r"((?: \d+)+)", r.stderr).group(1).split()]
                                      for name in ("s16 candidates", "s16 batches", "s8 candidates", "s8 batches"))
    return gen_golden.parse_dump(str(dump))[0], cand, batches, cand8, batches8


@pytest.mark.parametrize("which", ["plain", "reversed"])
@pytest.mark.parametrize("clip,qp,wpp", CASES)
def test_twin_equals_oracle(twins, clips, tmp_path, which, clip, qp, wpp):
    w, h, _, _ = CLIPS[clip]
    want_rec, want_ctus = reference(clips, clip, qp, wpp)
    (ctus, rec), cand, batches, cand8, batches8 = run_twin(twins[which], clips, clip, qp, wpp, tmp_path)
    print(f"{clip} qp{qp} wpp{wpp} {which}: 16x16 first passes by candidates {cand}, by batches {batches}; 8x8 first passes by candidates {cand8}, by batches {batches8}")
    common.assert_ctus_equal(ctus, want_ctus, f"{clip} qp{qp} wpp{wpp} {which}", (w, h))
    common.assert_rec_equal(want_rec, rec, w, h, "rec")
    assert sum(cand) > 0 and sum(cand) == sum(batches)
    if qp == 22:
        assert cand[3] > 0 and cand[4] > 0 and cand[5] > 0, f"PUs with 3, 4 and 5 candidates must all occur: {cand}"
        assert batches[2] > 0, f"some PU must take two batches (the twin counts the batch loop's iterations): {batches}"
        assert batches[1] == cand[3] + cand[4] and batches[2] == cand[5] + cand[6] and batches[3] == 0, f"a batch holds four, a later one three: {cand} {batches}"
        assert sum(cand8) > 0, f"8x8 first passes must occur: {cand8}"
        assert batches8 == [0, sum(cand8), 0, 0], f"every 8x8 first pass takes exactly one batch: {cand8} {batches8}"
        assert cand8[8] > 0 and sum(cand8[9:]) > 0, f"8x8 PUs with 8 and with more than 8 candidates must both occur: {cand8}"


def test_standalone_twin_under_address_and_undefined_sanitizers(clips, tmp_path):
    """the host twin as a stand-alone program built with -fsanitize=address,undefined (host code only) on the first clip at QP 22: no report, same dump as the plain twin's decisions"""
    exe = common.build_hostsim(tmp_path, "hostsim", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", exe="hostsim_san")
    want_rec, want_ctus = reference(clips, "128x128", 22, 1)
    (ctus, rec), cand, batches, cand8, batches8 = run_twin(exe, clips, "128x128", 22, 1, tmp_path)
    common.assert_ctus_equal(ctus, want_ctus, "sanitized twin", (128, 128))
    common.assert_rec_equal(want_rec, rec, 128, 128, "rec")
    assert cand[3] > 0 and cand[4] > 0 and cand[5] > 0 and batches[2] > 0
    assert cand8[8] > 0 and sum(cand8[9:]) > 0 and batches8 == [0, sum(cand8), 0, 0]
