"""GPU suite (-m gpu): the closing pass of a 64x64 intra PU taking its 32x32 TUs from the record of the winner's first pass (recur_intra_coding_qt,
pu64_record_tu / pu64_take_tu, hm355_core.h) on two launch shapes that reach it -- the team kernel with five wavefronts per CTU (one picture: the
helpers record and take on workspaces of their own) and the 12-search kernel with fewWaves == 0 (80 pictures) -- on the clips of
tests/test_large_pu_host.py: every whole CTU has one 64x64 PU; at QP 22 and 32 some of its TUs are taken from the record and some evaluated, at
QP 45 all are taken; 8 and 10 bits.  Slot 0 equals the oracle, all slots are equal; every case asserts the shape it ran."""
import numpy as np
import pytest

import common
import synth

pytestmark = pytest.mark.gpu

CLIPS = [(128, 128, 10, 1, 22), (128, 128, 10, 1, 32), (128, 128, 10, 1, 45), (192, 128, 8, 11, 32), (256, 128, 10, 5, 22)]     # width, height, bit depth, seed of synth.frame, QP
SHAPES = [(1, "team", 1, 5), (80, "search12", 0, 12)]                                                                           # pictures, kernel, fewWaves, wavefronts

_want = {}
def reference(clip):
    """oracle.compress of a clip, computed once and shared by the launch shapes"""
    import oracle
    if clip not in _want:
        w, h, bd, seed, qp = clip
        planes = synth.frame(w, h, bd, 0, seed)
        _want[clip] = (planes,) + tuple(oracle.compress(planes, bd, qp, 1))
    return _want[clip]


@pytest.mark.parametrize("n,kernel,few,waves", SHAPES)
@pytest.mark.parametrize("clip", CLIPS, ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}b_qp{c[4]}")
def test_hip_64x64_closing_pass_matches_oracle(built, clip, n, kernel, few, waves):
    import hm355
    w, h, bd, seed, qp = clip
    planes, want_rec, want_ctus = reference(clip)
    enc = hm355.Encoder(w, h, bd, 1, max_batch=n)
    res = enc.compress([planes] * n, qp)
    s = enc.last_launch_shape()
    enc.close()
    assert (s["kernel"], s["few_waves"], s["tickets"], s["waves"]) == (kernel, few, n * len(want_ctus), waves), s
    rec0, ctus0, stats0 = res[0]
    common.assert_ctus_equal(ctus0, want_ctus, f"{n} pictures, slot 0", (w, h))
    for c in range(3):
        assert np.array_equal(rec0[c], want_rec[c]), f"{n} pictures, slot 0: reconstruction plane {c}"
    for k in range(1, n):
        common.assert_ctus_equal(res[k][1], ctus0, f"{n} pictures, slot {k} vs slot 0")
        for c in range(3):
            assert np.array_equal(res[k][0][c], rec0[c]), f"{n} pictures, slot {k}: reconstruction plane {c}"
        assert res[k][2] == stats0, f"{n} pictures, slot {k}: picture totals"
