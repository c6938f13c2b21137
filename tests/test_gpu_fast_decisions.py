"""GPU suite (-m gpu): hm355_set_fast_decisions -- the reference's --ESD (early skip detection), --CFM (CBF fast mode) and --ECU (early CU) in the
search of P / B slices -- against clips the real reference encoded with the switches (tests/gen_golden_fast.py)."""
import os
import subprocess

import numpy as np
import pytest

import common
import synth
from test_fast_decisions_host import FAST_CASES, fast_flags

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


def _assert_slice(got, r, what):
    rec, ctus, ictus, stats = got
    common.assert_inter_ctus_equal(ctus, ictus, r["ctus"], what)
    for c in range(3):
        assert np.array_equal(rec[c], r["rec"][c]), f"{what}: reconstruction plane {c}"
    assert stats[0] == int(ctus["total_bits"].sum())


def _arm_dqp(hm, enc, r, bd):
    """cu_qp_delta clips: the CTU QPs of TEncCu::xComputeQP from the recorded activities, m_bEncodeDQP on entry"""
    q = r["dqp"]
    if q is None:
        return
    ctu_qp = hm.aq_ctu_qp(q["activity"], float(q["avg_activity"]), int(q["aq_range"]), int(r["qp"]), bd) if int(q["aq_range"]) > 0 else None
    enc.set_dqp(0, ctu_qp, int(q["dqp_flag_in"]))


@pytest.mark.parametrize("team", ["0", "1"])
@pytest.mark.parametrize("name", FAST_CASES)
def test_hip_fast_decisions_match_reference_fixture(hm, monkeypatch, name, team):
    """every P / B slice of the six clips through hm355_compress_slice_inter with the switches of the fixture: decisions, motion, coefficients,
    costs, reconstruction bit-exact.  HM355_TEAM=1 must not bring the wavefront teams back (they search speculatively)."""
    monkeypatch.setenv("HM355_TEAM", team)
    cfg, slices, finals = common.load_ldp_case(name)
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=1)
    enc.set_fast_decisions(*fast_flags(name))
    n_inter = 0
    for r in slices:
        if int(r["slice_type"]) == 2:
            continue
        planes = synth.frame(cfg["width"], cfg["height"], cfg["bit_depth"], int(r["poc"]), cfg["seed"])
        sp, refs = common.ldp_slice_inputs(r, finals)
        _arm_dqp(hm, enc, r, cfg["bit_depth"])
        _assert_slice(enc.compress_inter(planes, sp, refs), r, f"{name} POC {int(r['poc'])}")
        n_inter += 1
    assert n_inter >= 3
    enc.close()


def test_fast_decisions_are_sticky_and_can_be_switched_off(hm):
    """1/1/1 then 0/0/0: a clip of the default configuration equals its fixture; with ESD on it does not, and stays so for the next slice"""
    name = "ldp_192x128_8b_qp32"
    cfg, slices, finals = common.load_ldp_case(name)
    ps = [r for r in slices if int(r["slice_type"]) != 2]
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=1)

    def run(r):
        sp, refs = common.ldp_slice_inputs(r, finals)
        return enc.compress_inter(synth.frame(cfg["width"], cfg["height"], cfg["bit_depth"], int(r["poc"]), cfg["seed"]), sp, refs)

    enc.set_fast_decisions(1, 1, 1)
    enc.set_fast_decisions(0, 0, 0)
    for r in ps:
        _assert_slice(run(r), r, f"{name} POC {int(r['poc'])} after 1/1/1 -> 0/0/0")
    enc.set_fast_decisions(esd=1)
    for _ in range(2):                                     # no second call in between: the state belongs to the context
        with pytest.raises(AssertionError):
            _assert_slice(run(ps[0]), ps[0], "ESD")
    enc.close()


def test_i_slices_ignore_fast_decisions(hm):
    cfg, frames = common.load_case("small_128x128_10b_qp37")
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=cfg["frames"])
    enc.set_fast_decisions(1, 1, 1)
    planes = [synth.frame(cfg["width"], cfg["height"], cfg["bit_depth"], i, cfg["seed"]) for i in range(cfg["frames"])]
    for i, (got_rec, got_ctus, _) in enumerate(enc.compress(planes, cfg["qp"])):
        common.assert_ctus_equal(got_ctus, frames[i][0], f"frame {i}", (cfg["width"], cfg["height"]))
        common.assert_rec_equal(got_rec, frames[i][1], cfg["width"], cfg["height"], f"frame {i}")
    enc.close()


def test_fast_decisions_batch_equals_fixture(hm):
    """the P slices of the CFM clip in one hm355_compress_slices_inter call"""
    name = "fast_cfm_ldp_200x136_8b_qp30"
    cfg, slices, finals = common.load_ldp_case(name)
    ps = [r for r in slices if int(r["slice_type"]) == 1]
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=len(ps))
    enc.set_fast_decisions(*fast_flags(name))
    jobs = []
    for r in ps:
        sp, refs = common.ldp_slice_inputs(r, finals)
        jobs.append((synth.frame(cfg["width"], cfg["height"], cfg["bit_depth"], int(r["poc"]), cfg["seed"]), sp, refs))
    for r, got in zip(ps, enc.compress_inter_batch(jobs)):
        _assert_slice(got, r, f"{name} POC {int(r['poc'])} (batched)")
    enc.close()


@pytest.mark.parametrize("name,mode", [("fast_esd_ldp_192x128_8b_qp32", "ldp"), ("fast_all_ra_192x128_10b_qp32", "ra")])
def test_cpp_host_mirror_closed_loop_with_fast_decisions(tmp_path, name, mode):
    """hm355_encmain fast=<esd><cfm><ecu>: search -> deblocking -> SAO -> slice data -> device-resident reference -> the next search, every
    substream of every picture byte for byte as the reference wrote it with the same switches"""
    bd = {}
    cfg, slices, _ = common.load_ldp_case(name, bits=bd)
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump.bin"
    synth.write_yuv(str(yuv), cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["seed"])
    exe = os.path.join(common.ROOT, "hm-16.2_amd", "hm355_encmain")
    subprocess.run([exe, str(yuv), str(cfg["width"]), str(cfg["height"]), str(cfg["bit_depth"]), str(cfg["frames"]), str(int(slices[0]["qp"])), str(cfg["wpp"]),
                    str(dump), mode, "fast=%d%d%d" % fast_flags(name)], check=True)
    bits = common.read_mirror_bits(str(dump) + ".bits", cfg["frames"])
    assert len(slices) == cfg["frames"]
    for i, r in enumerate(slices):
        assert bits[i] == bd[int(r["poc"])]["substreams"], f"{name} POC {int(r['poc'])}: slice data bytes"


def test_set_fast_decisions_rejections_and_open_slice(hm):
    """a value other than 0 / 1; the setter while a slice is open (hm355_slice_begin_inter .. hm355_slice_end).  The slice opened with 1/1/1 runs
    to its end through hm355_run_ctus, and the setter is accepted again after hm355_slice_end."""
    w, h, bd, qp = 192, 128, 8, 34
    f0, cur = synth.frame(w, h, bd, 0, 17), synth.frame(w, h, bd, 1, 17)
    enc = hm.Encoder(w, h, bd, 1, max_batch=1)
    for bad in ((2, 0, 0), (0, -1, 0), (0, 0, 3)):
        with pytest.raises(RuntimeError):
            enc.set_fast_decisions(*bad)
    enc.upload(0, f0)
    enc.run(1, qp - 3)
    ref = enc.ref_from_slot(0, 0, False)
    sp = hm.inter_slice_params("P", qp, 0.4624 * 2.0 ** ((qp - 12) / 3.0), 1, (1, 0), np.zeros((2, 16), np.int32))
    enc.set_fast_decisions(1, 1, 1)
    enc.upload(0, cur)
    enc.set_dqp(0, None, 0)                                # a slice-resident search wants the slot armed: every CTU at the slice QP
    enc.slice_begin_inter(0, sp, {0: ref})
    with pytest.raises(RuntimeError):
        enc.set_fast_decisions(0, 0, 0)                    # a slice is open
    enc.run_ctus(0, 1, 0, enc.num_ctus)
    with pytest.raises(RuntimeError):
        enc.set_fast_decisions(0, 0, 0)                    # still open
    enc.slice_end(0)
    _, ctus, _ = enc.download(0)
    assert int(ctus["total_bits"].sum()) > 0
    enc.set_fast_decisions(0, 0, 0)                        # allowed again
    enc.ref_release(ref)
    enc.close()


def test_set_fast_decisions_rejected_while_a_launch_is_outstanding(hm):
    """between hm355_run_begin and hm355_run_wait the setter is refused (the launch has taken its Params), whether the kernel still runs or
    not; after the wait it is accepted and the launch's result is the one of an undisturbed run"""
    w, h, bd, qp = 128, 64, 8, 32
    planes = synth.frame(w, h, bd, 0, 1234)
    enc = hm.Encoder(w, h, bd, 1, max_batch=1)
    (want_rec, want_ctus, _), = enc.compress([planes], qp)
    enc.upload(0, planes)
    enc.run_begin(0, 0, 1, qp)
    with pytest.raises(RuntimeError):
        enc.set_fast_decisions(1, 1, 1)
    assert enc.run_wait(0) > 0
    enc.set_fast_decisions(1, 1, 1)
    got_rec, got_ctus, _ = enc.download(0)
    assert np.array_equal(got_ctus["total_bits"], want_ctus["total_bits"])
    for c in range(3):
        assert np.array_equal(got_rec[c], want_rec[c])
    enc.close()
