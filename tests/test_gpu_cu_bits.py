"""GPU suite (-m gpu): 2Nx2N intra CUs priced from the luma and chroma counts of their search (cu_bits_from_passes, hm355_core.h) on the three
launch shapes -- the 12-search kernel (HM355_TEAM=0), the team kernel, whose helpers evaluate CUs on workspaces of their own (HM355_TEAM=1), and
the 12-search kernel at fewWaves == 0 -- on the fresh inputs of tests/test_cu_bits_host.py: CTU records and reconstruction against the oracle."""
import numpy as np
import pytest

import common
import synth

pytestmark = pytest.mark.gpu

INPUTS = [(192, 128, 10, 12, 31), (200, 136, 8, 47, 32), (320, 192, 10, 32, 33)]      # width, height, bit depth, QP, seed of synth.frame

_want = {}
def reference(inp):
    """oracle.compress of an input (WaveFrontSynchro), computed once and shared by the launch shapes"""
    import oracle
    if inp not in _want:
        w, h, bd, qp, seed = inp
        planes = synth.frame(w, h, bd, 0, seed)
        _want[inp] = (planes,) + tuple(oracle.compress(planes, bd, qp, 1))
    return _want[inp]


def _assert_equals_oracle(res, inp, what):
    w, h = inp[:2]
    _, want_rec, want_ctus = reference(inp)
    rec, ctus, stats = res
    common.assert_ctus_equal(ctus, want_ctus, what, (w, h))
    for c in range(3):
        assert np.array_equal(rec[c], want_rec[c]), f"{what}: reconstruction plane {c}"
    assert stats[0] == int(want_ctus["total_bits"].sum()) and stats[2] == int(want_ctus["total_dist"].sum()), f"{what}: picture totals"


@pytest.mark.parametrize("team,kernel", [("0", "search12"), ("1", "team")])
@pytest.mark.parametrize("inp", INPUTS, ids=lambda i: f"{i[0]}x{i[1]}_{i[2]}b_qp{i[3]}")
def test_hip_cu_bits_from_passes_match_oracle(built, monkeypatch, inp, team, kernel):
    import hm355
    monkeypatch.setenv("HM355_TEAM", team)
    w, h, bd, qp, _ = inp
    planes = reference(inp)[0]
    enc = hm355.Encoder(w, h, bd, 1, max_batch=1)
    res, = enc.compress([planes], qp)
    s = enc.last_launch_shape()
    enc.close()
    assert s["kernel"] == kernel, s
    _assert_equals_oracle(res, inp, f"HM355_TEAM={team}")


def test_hip_cu_bits_from_passes_match_oracle_at_few_waves_0(built):
    """80 copies of the ragged 8-bit input in one launch: the 12-search kernel with fewWaves == 0, every workspace's parked counts in use"""
    import hm355
    inp = INPUTS[1]
    w, h, bd, qp, _ = inp
    planes, n = reference(inp)[0], 80
    enc = hm355.Encoder(w, h, bd, 1, max_batch=n)
    res = enc.compress([planes] * n, qp)
    s = enc.last_launch_shape()
    enc.close()
    assert (s["kernel"], s["few_waves"], s["waves"]) == ("search12", 0, 12), s
    _assert_equals_oracle(res[0], inp, "slot 0")
    for k in range(1, n):
        common.assert_ctus_equal(res[k][1], res[0][1], f"slot {k} vs slot 0")
        for c in range(3):
            assert np.array_equal(res[k][0][c], res[0][0][c]), f"slot {k}: reconstruction plane {c}"
        assert res[k][2] == res[0][2], f"slot {k}: picture totals"
