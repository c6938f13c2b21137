"""GPU suite (-m gpu): the launch shapes run_begin chooses beyond the few-picture ones (hm355_plan_launch, hm355_host_common.h) -- the 12-search
kernel with Params::fewWaves == 0 and more tickets than resident searches (what bench.py runs), both sides of the fewWaves threshold, P / B
batches on the team kernel and on the 12-search kernel at fewWaves == 0, cu_qp_delta at fewWaves == 0, and the one-CTU picture off the team
path -- against the reference's fixtures and the oracle.  Every test asserts through hm355_last_launch_shape that it ran the shape it was written for:
a retuned threshold makes it fail instead of quietly testing the team path again."""
import numpy as np
import pytest

import common
import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


def _assert_shape(enc, kernel, few_waves, tickets, waves=None):
    s = enc.last_launch_shape()
    assert (s["kernel"], s["few_waves"], s["tickets"]) == (kernel, few_waves, tickets), s
    assert s["waves"] == (12 if kernel == "search12" else waves), s
    assert s["workgroups"] >= 1
    return s


def _assert_same_search(a, b, what):
    """two (rec, ctus, stats) results of hm355_download are equal"""
    common.assert_ctus_equal(a[1], b[1], what)
    for k in range(3):
        assert np.array_equal(a[0][k], b[0][k]), f"{what}: reconstruction plane {k}"
    assert a[2] == b[2], f"{what}: picture totals"


def test_hip_i_launch_with_more_tickets_than_resident_searches(built, hm):
    """120 pictures of 7 x 4 CTUs (10 bit, partial CTUs right and below, WaveFrontSynchro) in one hm355_run: 3,360 tickets for 3,072 workspaces, so
    every workspace is used again by a CTU of another picture, on the fewWaves == 0 path.  Slot k holds frame k % 5 of the clip's seed: frame 0
    against the reference's fixture, frames 1 and 2 against the oracle, slots of equal content against each other."""
    import oracle
    cfg, frames = common.load_case("wpp_416x240_10b_qp32")
    w, h, bd, qp, n = cfg["width"], cfg["height"], cfg["bit_depth"], cfg["qp"], 120
    assert cfg["wpp"] == 1
    pics = [synth.frame(w, h, bd, f, cfg["seed"]) for f in range(5)]
    enc = hm.Encoder(w, h, bd, 1, max_batch=n)
    res = enc.compress([pics[k % 5] for k in range(n)], qp)
    s = _assert_shape(enc, "search12", 0, n * 28)
    assert s["tickets"] > 12 * s["workgroups"]
    enc.close()
    ctus, rec = frames[0]
    for k in range(0, n, 5):
        rec_k, ctus_k, stats = res[k]
        common.assert_ctus_equal(ctus_k, ctus, f"slot {k} (frame 0)", (w, h))
        common.assert_rec_equal(rec_k, rec, w, h, f"slot {k} (frame 0)")
        assert stats[0] == int(ctus["total_bits"].sum()) and stats[2] == int(ctus["total_dist"].sum())
    for f in (1, 2):
        want_rec, want_ctus = oracle.compress(pics[f], bd, qp, 1)
        common.assert_ctus_equal(res[f][1], want_ctus, f"slot {f} (frame {f})")
        for c in range(3):
            assert np.array_equal(res[f][0][c], want_rec[c]), f"slot {f} (frame {f}): reconstruction plane {c}"
    for k in range(5, n):
        _assert_same_search(res[k], res[k % 5], f"slot {k} vs slot {k % 5}")


def test_hip_i_launch_on_both_sides_of_the_few_waves_threshold(hm):
    """79 and 80 pictures of 4 x 3 CTUs (8 bit, WaveFrontSynchro) on the 12-search kernel: the last launch with fewWaves == 1 and the first with
    fewWaves == 0 (4x4 leaves through the general TU path); every slot equals the reference's fixture in both."""
    cfg, frames = common.load_case("wpp_256x192_8b_qp27")
    w, h, bd, qp = cfg["width"], cfg["height"], cfg["bit_depth"], cfg["qp"]
    assert cfg["wpp"] == 1
    pic = synth.frame(w, h, bd, 0, cfg["seed"])
    ctus, rec = frames[0]
    enc = hm.Encoder(w, h, bd, 1, max_batch=80)
    for n, few in ((79, 1), (80, 0)):
        res = enc.compress([pic] * n, qp)
        _assert_shape(enc, "search12", few, n * 12)
        for k in range(n):
            common.assert_ctus_equal(res[k][1], ctus, f"{n} pictures, slot {k}", (w, h))
            common.assert_rec_equal(res[k][0], rec, w, h, f"{n} pictures, slot {k}")
            assert res[k][2][0] == int(ctus["total_bits"].sum()) and res[k][2][2] == int(ctus["total_dist"].sum())
    enc.close()


def test_hip_p_slice_batches_at_few_waves_0_match_reference_fixture(hm):
    """The three P slices of the WPP low-delay clip (last CTU row cut: carry schedule, third dependency of a row start), each with its own
    references, 28 times in one batch (84 jobs: teams of nine wavefronts at fewWaves == 0) and 34 times (102 jobs: 12-search kernel at
    fewWaves == 0): every job equals its slice of the reference's fixture."""
    name = "ldpwpp_256x136_8b_qp30"
    cfg, slices, finals = common.load_ldp_case(name)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    assert cfg["wpp"] == 1 and h % 64 != 0
    ps = [r for r in slices if int(r["slice_type"]) == 1]
    assert len(ps) == 3
    base = []
    for r in ps:
        sp, refs = common.ldp_slice_inputs(r, finals)           # one ref_pics dict per POC, shared by its copies: uploaded once
        base.append((synth.frame(w, h, bd, int(r["poc"]), cfg["seed"]), sp, refs))
    enc = hm.Encoder(w, h, bd, 1, max_batch=102)
    for copies, kernel in ((28, "team"), (34, "search12")):
        got = enc.compress_inter_batch([base[k % 3] for k in range(3 * copies)])
        _assert_shape(enc, kernel, 0, 3 * copies * enc.num_ctus, waves=9)
        for k, (rec, ctus, ictus, stats) in enumerate(got):
            r = ps[k % 3]
            common.assert_inter_ctus_equal(ctus, ictus, r["ctus"], f"{3 * copies} jobs, job {k} (POC {int(r['poc'])})")
            for c in range(3):
                assert np.array_equal(rec[c], r["rec"][c]), f"{3 * copies} jobs, job {k}: reconstruction plane {c}"
            assert stats[0] == int(ctus["total_bits"].sum())
    enc.close()


@pytest.mark.parametrize("name,slice_type", [("edge_ldp_136x72_8b_qp0", 1), ("edge_ldb_136x72_10b_qp2", 0)])
def test_hip_low_qp_slice_batches_at_few_waves_0_match_reference_fixture(hm, name, slice_type):
    """The three P slices of the QP-0 clip and the three B slices of the 10-bit QP-2 clip (slice QPs 2..5, levels of several hundred in the inter
    pictures), each with its own references, in one batch of 1,280 jobs: without WaveFrontSynchro a picture offers one CTU at a time, so this is the
    smallest batch hm355_plan_launch gives Params::fewWaves == 0, and past 1,024 streams it runs on the 12-search kernel -- the large levels go
    through its lane code.  The first copy of each slice equals the reference's fixture; every other copy equals the first."""
    cfg, slices, finals = common.load_ldp_case(name)
    w, h, bd, n = cfg["width"], cfg["height"], cfg["bit_depth"], 1280
    assert cfg["wpp"] == 0
    ps = [r for r in slices if int(r["slice_type"]) == slice_type]
    assert len(ps) == 3 and len(slices) == 4
    base = []
    for r in ps:
        sp, refs = common.ldp_slice_inputs(r, finals)           # one ref_pics dict per POC, shared by its copies: uploaded once
        base.append((synth.frame(w, h, bd, int(r["poc"]), cfg["seed"]), sp, refs))
    enc = hm.Encoder(w, h, bd, 0, max_batch=n)
    got = enc.compress_inter_batch([base[k % 3] for k in range(n)])
    _assert_shape(enc, "search12", 0, n * enc.num_ctus)
    enc.close()
    for k in range(3):
        rec, ctus, ictus, stats = got[k]
        r = ps[k]
        common.assert_inter_ctus_equal(ctus, ictus, r["ctus"], f"job {k} (POC {int(r['poc'])})")
        for c in range(3):
            assert np.array_equal(rec[c], r["rec"][c]), f"job {k}: reconstruction plane {c}"
        assert stats[0] == int(ctus["total_bits"].sum())
    for k in range(3, n):
        first = got[k % 3]
        assert got[k][1].tobytes() == first[1].tobytes() and got[k][2].tobytes() == first[2].tobytes(), f"job {k} differs from job {k % 3}"
        for c in range(3):
            assert np.array_equal(got[k][0][c], first[0][c]), f"job {k}: reconstruction plane {c} differs from job {k % 3}"
        assert got[k][3] == first[3], f"job {k}: picture totals"


def test_hip_b_slice_batch_under_wpp_at_few_waves_0_matches_oracle(built, hm):
    """A B slice under WaveFrontSynchro (192x136, 10 bit, two pictures per list, built as in test_hip_inter_matches_oracle_on_fresh_inputs), 100 copies
    in one batch: 12-search kernel at fewWaves == 0; job 0 equals the oracle, all jobs are equal, some partition is bi-predicted."""
    import oracle
    w, h, bd, wpp, qp, seed, copies = 192, 136, 10, 1, 30, 77, 100
    enc = hm.Encoder(w, h, bd, wpp, max_batch=copies)
    n = enc.num_ctus
    res = enc.compress([synth.frame(w, h, bd, f, seed) for f in (0, 4)], qp)
    mot = np.zeros(n, [("pred_mode", "u1", 256), ("mv0", "<i2", (256, 2)), ("ref_idx0", "i1", 256), ("mv1", "<i2", (256, 2)), ("ref_idx1", "i1", 256)])
    mot["pred_mode"] = 1; mot["ref_idx0"] = -1; mot["ref_idx1"] = -1
    zero = np.zeros((2, 16), np.int32)
    finals = {poc: {"poc": poc, "slice_type": 2, "rec": res[k][0], "motion": mot, "num_ref_idx": (0, 0), "ref_poc": zero, "ref_long_term": zero}
              for k, poc in enumerate((0, 4))}
    ref_poc = np.zeros((2, 16), np.int32)
    ref_poc[0, :2] = (0, 4); ref_poc[1, :2] = (4, 0)
    lam = 0.4624 * 2.0 ** ((qp + 2 - 12) / 3.0) * 2.0
    sp = hm.inter_slice_params("B", qp + 2, lam, 2, (2, 2), ref_poc, col_from_l0=0, check_ldc=0)
    srec = dict(sp, weight_cb=sp["chroma_weight"])           # as an 'S' record, for the oracle and ldp_slice_inputs
    cur = synth.frame(w, h, bd, 2, seed)
    want_rec, want_ctus, want_ictus = oracle.compress_inter(cur, bd, srec, finals, wpp=wpp)
    _, refs = common.ldp_slice_inputs(srec, finals)
    got = enc.compress_inter_batch([(cur, sp, refs)] * copies)
    _assert_shape(enc, "search12", 0, copies * n)
    enc.close()
    rec, ctus, ictus, _ = got[0]
    for f in ("total_bits", "total_dist", "total_cost", "depth", "part_size", "pred_mode", "tr_idx", "cbf", "tskip", "coeff_y", "coeff_cb", "coeff_cr"):
        assert np.array_equal(ctus[f], want_ctus[f]), f"job 0: {f} differs from the oracle"
    for f in ("skip", "merge_flag", "merge_idx", "inter_dir", "mv", "mvd", "ref_idx", "mvp_idx", "mvp_num"):
        assert np.array_equal(ictus[f], want_ictus[f]), f"job 0: {f} differs from the oracle"
    for c in range(3):
        assert np.array_equal(rec[c], want_rec[c]), f"job 0: reconstruction plane {c} differs from the oracle"
    assert (ictus["inter_dir"] == 3).any(), "no bi-predicted partition"
    for k in range(1, copies):
        assert got[k][1].tobytes() == ctus.tobytes() and got[k][2].tobytes() == ictus.tobytes(), f"job {k} differs from job 0"
        for c in range(3):
            assert np.array_equal(got[k][0][c], rec[c]), f"job {k}: reconstruction plane {c} differs from job 0"
        assert got[k][3] == got[0][3]


def test_hip_cu_qp_delta_at_few_waves_0_matches_reference(hm):
    """The two AdaptiveQP I pictures of the WPP clip alternating in 80 slots, every slot armed as test_hip_cu_qp_delta_matches_reference arms its one
    (hm355_preanalyze -> activities -> CTU QPs -> hm355_set_dqp), one hm355_run: 12-search kernel at fewWaves == 0.  Decisions, coefficients,
    costs, reconstruction, m_phQP inside the picture and m_bEncodeDQP of every slot equal the reference's fixture.  hm355_last_launch_shape reports
    the first launch of the call, so the rows dqp_verify_rows may search again with one-slot launches do not hide the 80-slot launch."""
    name = "aq_iwpp_320x200_10b_qp27"
    cfg, slices, _ = common.load_ldp_case(name)
    w, h, bd, n = cfg["width"], cfg["height"], cfg["bit_depth"], 80
    assert cfg["wpp"] == 1 and len(slices) == 2 and all(int(r["slice_type"]) == 2 for r in slices)
    enc = hm.Encoder(w, h, bd, 1, max_batch=n)
    pics = [synth.frame(w, h, bd, int(r["poc"]), cfg["seed"]) for r in slices]
    for k in range(n):
        r = slices[k % 2]; q = r["dqp"]
        enc.upload(k, pics[k % 2])
        assert int(q["aq_range"]) > 0
        act, avg = hm.aq_activities(enc.preanalyze(k))
        assert np.array_equal(act, q["activity"]) and avg == float(q["avg_activity"]), f"slot {k}: activities"
        enc.set_dqp(k, hm.aq_ctu_qp(act, avg, int(q["aq_range"]), int(r["qp"]), bd), int(q["dqp_flag_in"]))
    sl = (hm.SliceDesc * n)(*[hm.SliceDesc(2, int(slices[k % 2]["qp"]), float(slices[k % 2]["lambda"]), float(slices[k % 2]["weight_cb"])) for k in range(n)])
    enc._check(enc.lib.hm355_run(enc.h_, n, sl), "hm355_run")
    _assert_shape(enc, "search12", 0, n * enc.num_ctus)
    want = [common.split_fixture_ctus(r["ctus"])[0] for r in slices]
    m = common.inside_mask(enc.num_ctus, w, h)
    for k in range(n):
        r = slices[k % 2]; q = r["dqp"]
        rec, ctus, _ = enc.download(k)
        common.assert_ctus_equal(ctus, want[k % 2], f"slot {k} (POC {int(r['poc'])})")
        for c in range(3):
            assert np.array_equal(rec[c], r["rec"][c]), f"slot {k}: reconstruction plane {c}"
        qp, flag = enc.get_dqp(k)
        assert np.array_equal(qp[m], q["qp"][m]), f"slot {k}: m_phQP differs in CTUs {np.nonzero(((qp != q['qp']) & m).any(axis=1))[0][:8]}"
        assert flag == int(q["dqp_flag_out"]), f"slot {k}: m_bEncodeDQP after the slice"
    enc.close()


# ---- the one-CTU picture with max_batch 1: nine team workspaces used to be all the lane had, and a launch off the team path got no workgroup ----
ONE_CTU = dict(w=64, h=64, bd=8, qp=22, seed=13)      # the P slice: four 32x32 CUs, half of the partitions with a motion vector


@pytest.fixture(scope="module")
def one_ctu(built, hm):
    """the oracle's I slice of the 64x64 clip's frame 0 and its P slice of frame 1 with that I reconstruction as the only reference, per wpp;
    computed once, read-only"""
    import oracle
    w, h, bd, qp, seed = (ONE_CTU[k] for k in ("w", "h", "bd", "qp", "seed"))
    out = {}
    for wpp in (0, 1):
        i_pic, p_pic = synth.frame(w, h, bd, 0, seed), synth.frame(w, h, bd, 1, seed)
        i_rec, i_ctus = oracle.compress(i_pic, bd, qp, wpp)
        mot = np.zeros(1, [("pred_mode", "u1", 256), ("mv0", "<i2", (256, 2)), ("ref_idx0", "i1", 256), ("mv1", "<i2", (256, 2)), ("ref_idx1", "i1", 256)])
        mot["pred_mode"] = 1; mot["ref_idx0"] = -1; mot["ref_idx1"] = -1
        zero = np.zeros((2, 16), np.int32)
        finals = {0: {"poc": 0, "slice_type": 2, "rec": i_rec, "motion": mot, "num_ref_idx": (0, 0), "ref_poc": zero, "ref_long_term": zero}}
        lam = 0.4624 * 2.0 ** ((qp + 2 - 12) / 3.0) * 2.0
        sp = hm.inter_slice_params("P", qp + 2, lam, 1, (1, 0), zero)
        srec = dict(sp, weight_cb=sp["chroma_weight"])
        p_want = oracle.compress_inter(p_pic, bd, srec, finals, wpp=wpp)
        _, refs = common.ldp_slice_inputs(srec, finals)
        out[wpp] = dict(i_pic=i_pic, p_pic=p_pic, i_want=(i_rec, i_ctus), sp=sp, refs=refs, p_want=p_want)
    return out


@pytest.mark.parametrize("wpp", [0, 1])
def test_hip_one_ctu_picture_without_teams_matches_oracle(hm, monkeypatch, one_ctu, wpp):
    """64x64, max_batch 1, HM355_TEAM=0: the I slice and a P slice (one reference: that I reconstruction) on the 12-search kernel equal the oracle"""
    monkeypatch.setenv("HM355_TEAM", "0")
    d = one_ctu[wpp]
    enc = hm.Encoder(ONE_CTU["w"], ONE_CTU["h"], ONE_CTU["bd"], wpp, max_batch=1)
    (rec, ctus, stats), = enc.compress([d["i_pic"]], ONE_CTU["qp"])
    _assert_shape(enc, "search12", 1, 1)
    common.assert_ctus_equal(ctus, d["i_want"][1], "I slice")
    for c in range(3):
        assert np.array_equal(rec[c], d["i_want"][0][c]), f"I slice: reconstruction plane {c}"
    assert stats[0] == int(ctus["total_bits"].sum()) and stats[2] == int(ctus["total_dist"].sum())
    rec, ctus, ictus, stats = enc.compress_inter(d["p_pic"], d["sp"], d["refs"])
    _assert_shape(enc, "search12", 1, 1)
    enc.close()
    want_rec, want_ctus, want_ictus = d["p_want"]
    for f in ("total_bits", "total_dist", "total_cost", "depth", "part_size", "pred_mode", "tr_idx", "cbf", "tskip", "coeff_y", "coeff_cb", "coeff_cr"):
        assert np.array_equal(ctus[f], want_ctus[f]), f"P slice: {f} differs"
    for f in ("skip", "merge_flag", "merge_idx", "inter_dir", "mv", "mvd", "ref_idx", "mvp_idx", "mvp_num"):
        assert np.array_equal(ictus[f], want_ictus[f]), f"P slice: {f} differs"
    for c in range(3):
        assert np.array_equal(rec[c], want_rec[c]), f"P slice: reconstruction plane {c}"
    assert stats[0] == int(ctus["total_bits"].sum())


@pytest.mark.parametrize("wpp", [0, 1])
def test_hip_one_ctu_p_slice_with_fast_decisions_is_searched(hm, one_ctu, wpp):
    """the product's own route off the team path: a P slice of the one-CTU picture after hm355_set_fast_decisions(1, 1, 1) gets a workgroup of the
    12-search kernel and a result (the oracle has no switches: no parity claim)"""
    d = one_ctu[wpp]
    enc = hm.Encoder(ONE_CTU["w"], ONE_CTU["h"], ONE_CTU["bd"], wpp, max_batch=1)
    enc.set_fast_decisions(1, 1, 1)
    rec, ctus, ictus, stats = enc.compress_inter(d["p_pic"], d["sp"], d["refs"])
    s = _assert_shape(enc, "search12", 1, 1)
    assert s["workgroups"] >= 1
    enc.close()
    assert stats[0] == int(ctus["total_bits"].sum()) and stats[2] == int(ctus["total_dist"].sum())
    assert int(ctus["total_bits"].sum()) > 0
