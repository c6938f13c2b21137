"""GPU suite (-m gpu): the LCU-level rate control of SURVEY 8f n4, stage 2 (include/hm355.h: hm355_set_ctu_rc, hm355_slice_begin*, hm355_run_ctus,
hm355_ctu_rc_feedback, hm355_intra_cost) against the clips the reference encoded with --RateControl=1 --LCULevelRateControl=1: given the lambda and
the QP the reference's rate model handed every CTU ('L' records), the device reproduces the whole per-picture pipeline bit for bit -- whole slices,
one CTU per call with the rate model's inputs read back in between, one CTU row per call, and two slots in one launch."""
import numpy as np
import pytest

import common
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


def _want_feedback(r, w, h):
    """(bits, QP) TEncSlice.cpp:861-887 hands updateAfterCTU, from the fixture: getTotalBits(), getQP(0) -- or -999 when no partition inside the
    picture is coded other than skip"""
    want = r["ctus"]
    m = common.inside_mask(len(want), w, h)
    skip = want["skip"] if "skip" in want.dtype.names else np.zeros_like(want["pred_mode"])
    coded = (m & (want["pred_mode"] != 2) & (skip == 0)).any(axis=1)
    return want["total_bits"].astype(np.int64), np.where(coded, r["dqp"]["qp"][:, 0].astype(np.int64), -999)


def _replay(hm, name, mode, slots=1, setup=None):
    """The clip in coding order with the closed loop on slot 0 (search -> deblocking -> SAO -> slice data -> device-resident reference).
    mode "whole": hm355_set_ctu_rc for every CTU, then the whole-slice search (hm355_run / compress_inter); "ctu": one CTU per hm355_run_ctus call
    with hm355_set_ctu_rc before and hm355_ctu_rc_feedback after it; "row": one CTU row per call.  slots > 1: the same picture in every slot, driven
    by hm355_run_ctus(first_slot=0, n=slots, ...); every slot is compared with the fixture.  setup(enc): called once on the new context before the
    first picture (the sticky setters of a clip encoded with further options)."""
    saod, bitd = {}, {}
    cfg, slices, finals = common.load_ldp_case(name, sao=saod, bits=bitd)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    wc = (w + 63) // 64
    rate = np.zeros((3, 8), np.float64)
    enc = hm.Encoder(w, h, bd, cfg["wpp"], max_batch=slots)
    if setup is not None:
        setup(enc)
    n = enc.num_ctus
    dev_refs = {}
    for r in slices:
        st, poc, q, lcu = int(r["slice_type"]), int(r["poc"]), r["dqp"], r["lcu_rc"]
        what = f"{name} POC {poc} ({mode}, {slots} slot(s))"
        ctu_qp, ctu_lam = np.asarray(lcu["ctu_qp"]).astype(np.int8), np.asarray(lcu["ctu_lambda"], np.float64)
        planes = synth.frame(w, h, bd, poc, cfg["seed"])
        want_bits, want_qp = _want_feedback(r, w, h)
        sp = refs = None
        if st != 2:
            sp, _ = common.ldp_slice_inputs(r, finals)
            refs = {int(p): dev_refs[int(p)] for l in range(2) for p in r["ref_poc"][l][:r["num_ref_idx"][l]]}
        for s in range(slots):
            enc.set_dqp(s, None, int(q["dqp_flag_in"]))
        if mode == "whole":
            enc.set_ctu_rc(0, 0, ctu_qp, ctu_lam)
            if st == 2:
                enc.upload(0, planes)
                sl = (hm.SliceDesc * 1)(hm.SliceDesc(2, int(r["qp"]), float(r["lambda"]), float(r["weight_cb"])))
                enc._check(enc.lib.hm355_run(enc.h_, 1, sl), "hm355_run")
            else:
                enc.compress_inter(planes, sp, refs)
            fb = enc.ctu_rc_feedback(0, 0, n)
            assert np.array_equal(fb["bits"], want_bits) and np.array_equal(fb["qp"], want_qp), f"{what}: rate control feedback of the whole slice"
        else:
            for s in range(slots):
                enc.upload(s, planes)
                if st == 2:
                    enc.slice_begin(s, int(r["qp"]), float(r["lambda"]), float(r["weight_cb"]))
                else:
                    enc.slice_begin_inter(s, sp, refs)
            step = 1 if mode == "ctu" else wc
            for a in range(0, n, step):
                k = min(step, n - a)
                for s in range(slots):
                    enc.set_ctu_rc(s, a, ctu_qp[a:a + k], ctu_lam[a:a + k])
                enc.run_ctus(0, slots, a, k)
                for s in range(slots):
                    fb = enc.ctu_rc_feedback(s, a, k)
                    assert np.array_equal(fb["bits"], want_bits[a:a + k]), f"{what} slot {s}: bits of CTUs {a}..{a + k - 1}"
                    assert np.array_equal(fb["qp"], want_qp[a:a + k]), f"{what} slot {s}: QP of CTUs {a}..{a + k - 1} for updateAfterCTU"
            for s in range(slots):
                enc.slice_end(s)
        for s in range(slots):
            rec, ctus, _ = enc.download(s)
            if st == 2:
                common.assert_ctus_equal(ctus, common.split_fixture_ctus(r["ctus"])[0], f"{what} slot {s}")
            else:
                common.assert_inter_ctus_equal(ctus, enc.download_inter(s), r["ctus"], f"{what} slot {s}")
            for c in range(3):
                assert np.array_equal(rec[c], r["rec"][c]), f"{what} slot {s}: pre-deblocking reconstruction plane {c}"
            qp, flag = enc.get_dqp(s)
            m = common.inside_mask(n, w, h)
            assert np.array_equal(qp[m], q["qp"][m]), f"{what} slot {s}: m_phQP differs in CTUs {np.nonzero(((qp != q['qp']) & m).any(axis=1))[0][:8]}"
            assert flag == int(q["dqp_flag_out"]), f"{what} slot {s}: m_bEncodeDQP after the slice"
        enc.deblock_run([(st, int(r["qp"]), r["ref_poc"])])
        (en3, _), = enc.sao_run([dict(qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), depth=saod[poc]["depth"], disabled_rate=rate,
                                      chroma_weight=float(r["weight_cb"]), **{"lambda": float(r["lambda"])})])
        (subs, nxt, bins), = enc.encode_slices_run([dict(slice_type=st, qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), num_ref_idx=r["num_ref_idx"],
                                                         mvd_l1_zero=int(r["mvd_l1_zero"]), max_merge_cand=int(r["max_merge_cand"]), sao_enabled=(en3[0], en3[1]))])
        assert subs == bitd[poc]["substreams"], f"{what}: slice data bytes differ"
        assert (nxt, bins) == (bitd[poc]["next_cabac_init_type"], bitd[poc]["num_bins"]), f"{what}: next context table / bin count"
        fin, _, _ = enc.download(0, want_ctus=False)
        for c in range(3):
            assert np.array_equal(fin[c], finals[poc]["rec"][c]), f"{what}: finished picture plane {c}"
        dev_refs[poc] = enc.ref_from_slot(0, poc, st != 2, r["num_ref_idx"], r["ref_poc"], r["ref_long_term"])
    for ref in dev_refs.values():
        enc.ref_release(ref)
    enc.close()
    return len(slices)


@pytest.mark.parametrize("team", ["0", "1"])
@pytest.mark.parametrize("name", common.LCU_RC_CASES)
def test_lcu_rate_control_whole_slices_match_reference(hm, monkeypatch, name, team):
    """a lambda and a QP per CTU (hm355_set_ctu_rc) through the whole-slice searches, one wavefront per CTU and teams"""
    monkeypatch.setenv("HM355_TEAM", team)
    assert _replay(hm, name, "whole") >= 2


@pytest.mark.parametrize("name", common.LCU_RC_CASES)
def test_lcu_rate_control_one_ctu_per_call_matches_reference(hm, name):
    """the host in the loop: hm355_set_ctu_rc(a), hm355_run_ctus(a, 1), hm355_ctu_rc_feedback(a) -- the bits and QP updateAfterCTU takes"""
    assert _replay(hm, name, "ctu") >= 2


def test_lcu_rate_control_one_row_per_call_matches_reference(hm):
    """WaveFrontSynchro: every call starts at a row start, whose m_bEncodeDQP comes from the CTU the previous call finished"""
    assert _replay(hm, "rc2_ldp_256x128_8b", "row") >= 2


@pytest.mark.parametrize("name", ["rc2_i_256x192_10b", "rc2_ldp_256x128_8b"])
def test_lcu_rate_control_two_slots_in_one_launch(hm, name):
    assert _replay(hm, name, "ctu", slots=2) >= 2


def test_lcu_rate_control_row_starts_take_the_real_flag(hm):
    """WaveFrontSynchro: the first CTU of a row takes m_bEncodeDQP from the last CTU of the row above.  A whole-slice search starts rows on the
    guess "clear" and searches again from a row whose guess was wrong; hm355_run_ctus uses the real value of a CTU an earlier call finished.  A
    synthetic P picture at high QP, static on the right so that row-end CTUs are all skip (they leave the flag set), searched one CTU and one row
    per call, must equal the whole-slice search: decisions, motion, coefficients, costs, reconstruction, m_phQP and the flag after the slice."""
    w, h, bd, qp = 384, 256, 8, 46
    f0, f1 = synth.frame(w, h, bd, 0, 91), synth.frame(w, h, bd, 1, 91)
    cur = [p.copy() for p in f0]
    for k, s in enumerate((64, 32, 32)):                                         # only the first CTU column changes
        cur[k][:, :s] = f1[k][:, :s]
    enc = hm.Encoder(w, h, bd, 1, max_batch=1)
    n, wc = enc.num_ctus, (w + 63) // 64
    enc.upload(0, f0)
    enc.run(1, qp - 4)
    enc.deblock_run([(2, qp - 4, np.zeros((2, 16), np.int32))])
    ref = enc.ref_from_slot(0, 0, False)
    lam = 0.4624 * 2.0 ** ((qp - 12) / 3.0)
    sp = hm.inter_slice_params("P", qp, lam, 1, (1, 0), np.zeros((2, 16), np.int32))
    rng = np.random.default_rng(3)
    qps = (qp + rng.integers(-3, 4, n)).clip(0, 51).astype(np.int8)
    lams = lam * 2.0 ** ((qps.astype(np.float64) - qp) / 3.0)
    enc.set_dqp(0, None, 0)
    enc.set_ctu_rc(0, 0, qps, lams)
    want_rec, want, want_i, _ = enc.compress_inter(cur, sp, {0: ref})
    want_qp, want_flag = enc.get_dqp(0)
    row_end_skip = [y for y in range(h // 64 - 1) if not want["cbf"][y * wc + wc - 1].any()]
    assert row_end_skip, "the picture should have a row whose last CTU codes no block (it leaves m_bEncodeDQP set for the next row start)"
    for step in (1, wc):
        enc.upload(0, cur)
        enc.set_dqp(0, None, 0)
        enc.slice_begin_inter(0, sp, {0: ref})
        for a in range(0, n, step):
            enc.set_ctu_rc(0, a, qps[a:a + step], lams[a:a + step])
            enc.run_ctus(0, 1, a, step)
        enc.slice_end(0)
        rec, ctus, _ = enc.download(0)
        common.assert_ctus_equal(ctus, want, f"{step} CTU(s) per call")
        got_i = enc.download_inter(0)
        for f in got_i.dtype.names:
            assert np.array_equal(got_i[f], want_i[f]), f"{step} CTU(s) per call: {f}"
        for c in range(3):
            assert np.array_equal(rec[c], want_rec[c]), f"{step} CTU(s) per call: reconstruction plane {c}"
        got_qp, got_flag = enc.get_dqp(0)
        assert np.array_equal(got_qp, want_qp) and got_flag == want_flag, f"{step} CTU(s) per call: m_phQP / m_bEncodeDQP"
    enc.ref_release(ref)
    enc.close()


def _intra_cost_np(y, bd):
    """TEncSlice::calCostSliceI restated: per CTU the 8x8 Hadamard costs (sum |c| - |DC|, (s + 2) >> 2) of the whole 8x8 blocks inside the
    picture, then (sum + offset) >> (bd - 8)"""
    h, w = y.shape
    hb, wb = h // 8, w // 8
    H = np.array([[1]], np.int64)
    for _ in range(3):
        H = np.block([[H, H], [H, -H]])
    blk = y[:hb * 8, :wb * 8].astype(np.int64).reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3)
    c = np.einsum("ij,abjk,lk->abil", H, blk, H)
    s = np.abs(c).sum(axis=(2, 3)) - np.abs(c[:, :, 0, 0])
    had = (s + 2) >> 2
    wc, hc = (w + 63) // 64, (h + 63) // 64
    pad = np.zeros((hc * 8, wc * 8), np.int64)
    pad[:hb, :wb] = had
    tot = pad.reshape(hc, 8, wc, 8).sum(axis=(1, 3)).reshape(-1)
    shift = bd - 8
    return (tot + ((1 << (shift - 1)) if shift > 0 else 0)) >> shift


def _intra_cost_dev(hm, planes, bd):
    h, w = planes[0].shape
    enc = hm.Encoder(w, h, bd, 0, max_batch=1)
    enc.upload(0, planes)
    got = enc.intra_cost(0)
    enc.close()
    return got


def test_intra_cost_matches_restatement(hm):
    """hm355_intra_cost (gfx950 kernel) against a numpy restatement: the pictures of the all-intra rate control clip (10-bit), a ragged 8-bit
    200x136 picture, a 3840x2160 10-bit picture; known answers: a flat picture costs 0, and one 10-bit picture checks the rounding offset"""
    cfg, slices, _ = common.load_ldp_case("rc2_i_256x192_10b")
    for r in slices:
        planes = synth.frame(cfg["width"], cfg["height"], cfg["bit_depth"], int(r["poc"]), cfg["seed"])
        assert np.array_equal(_intra_cost_dev(hm, planes, 10), _intra_cost_np(planes[0], 10)), f"POC {int(r['poc'])}"
    planes = synth.frame(200, 136, 8, 0, 77)
    assert np.array_equal(_intra_cost_dev(hm, planes, 8), _intra_cost_np(planes[0], 8))
    rng = np.random.default_rng(4)
    planes = [rng.integers(0, 1024, (2160, 3840)).astype(np.uint16), rng.integers(0, 1024, (1080, 1920)).astype(np.uint16),
              rng.integers(0, 1024, (1080, 1920)).astype(np.uint16)]
    assert np.array_equal(_intra_cost_dev(hm, planes, 10), _intra_cost_np(planes[0], 10))
    flat = [np.full((136, 200), 77, np.uint16), np.full((68, 100), 128, np.uint16), np.full((68, 100), 128, np.uint16)]
    assert np.array_equal(_intra_cost_dev(hm, flat, 8), np.zeros(12, np.int32))
    # one sample 3 at (0, 0), zeros elsewhere: every coefficient of that block is +-3, (63 * 3 + 2) >> 2 = 47, and (47 + 2) >> 2 = 12 (without the
    # 10-bit rounding offset: 11)
    one = [np.zeros((128, 128), np.uint16), np.zeros((64, 64), np.uint16), np.zeros((64, 64), np.uint16)]
    one[0][0, 0] = 3
    assert list(_intra_cost_dev(hm, one, 10)) == [12, 0, 0, 0]


def _rejects(enc, fn, *args):
    with pytest.raises(RuntimeError) as ei:
        fn(*args)
    msg = str(ei.value)
    assert "rc=-1" in msg and msg.split(":", 1)[1].strip(), msg


def test_lcu_rate_control_rejections(hm):
    """HM355_ERR_ARG with a message, and the context usable afterwards"""
    cfg, slices, finals = common.load_ldp_case("rc2_ldp_256x128_8b")
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    enc = hm.Encoder(w, h, bd, cfg["wpp"], max_batch=1)
    n = enc.num_ctus
    _rejects(enc, enc.set_ctu_rc, 0, 0, [30])                                   # slot not armed
    r0 = slices[0]
    planes = synth.frame(w, h, bd, int(r0["poc"]), cfg["seed"])
    enc.upload(0, planes)
    _rejects(enc, enc.slice_begin, 0, int(r0["qp"]), float(r0["lambda"]), float(r0["weight_cb"]))   # a slice on a slot not armed
    enc.set_dqp(0, None, 0)
    for lam in (0.0, -1.0, float("nan"), float("inf"), 1e12, 1e-300):
        _rejects(enc, enc.set_ctu_rc, 0, 0, [30], [lam])
    _rejects(enc, enc.set_ctu_rc, 0, 0, [-1], [10.0])                           # 8-bit: QP in [0, 51]
    _rejects(enc, enc.set_ctu_rc, 0, 0, [52], [10.0])
    _rejects(enc, enc.set_ctu_rc, 0, n - 1, [30, 30], [10.0, 10.0])             # past numCtus
    _rejects(enc, enc.run_ctus, 0, 1, 0, 1)                                     # no slice_begin
    _rejects(enc, enc.ctu_rc_feedback, 0, 0, 1)                                 # nothing searched since the upload
    enc.slice_begin(0, int(r0["qp"]), float(r0["lambda"]), float(r0["weight_cb"]))
    _rejects(enc, enc.set_dqp, 0, None, 0)                                      # re-arming an open slice: slice_begin -> set_dqp -> set_ctu_rc
    _rejects(enc, enc.set_dqp, 0, None, 0, 0)
    enc.set_ctu_rc(0, 0, [int(r0["qp"])], [float(r0["lambda"])])                # the slice's state is still the one it was begun with
    _rejects(enc, enc.run_ctus, 0, 1, 1, 1)                                     # a gap
    enc.run_ctus(0, 1, 0, 1)
    _rejects(enc, enc.run_ctus, 0, 1, 0, 1)                                     # a repeat
    _rejects(enc, enc.set_ctu_rc, 0, 0, [30], [10.0])                           # a CTU already searched
    enc.slice_end(0)
    p = next(r for r in slices if int(r["slice_type"]) != 2)
    sp, host_refs = common.ldp_slice_inputs(p, finals)
    _rejects(enc, enc.slice_begin_inter, 0, sp, host_refs)                      # host reference pictures
    # still usable: a whole I slice under the rate control's values
    enc.set_ctu_rc(0, 0, np.full(n, int(r0["qp"]), np.int8), np.full(n, float(r0["lambda"])))
    enc.slice_begin(0, int(r0["qp"]), float(r0["lambda"]), float(r0["weight_cb"]))
    enc.run_ctus(0, 1, 0, n)
    assert len(enc.ctu_rc_feedback(0, 0, n)) == n
    enc.slice_end(0)
    enc.close()
