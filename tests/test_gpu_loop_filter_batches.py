"""Batched loop filters with a different descriptor in every slot: hm355_run, hm355_deblock_run, hm355_sao_run and hm355_encode_slices_run take n
descriptors and run the pictures of a batch side by side in one launch each.  Here every slot has its own QP (both sides of deblocking's beta == 0
at QP 16, the end of the tc table at QP 51), its own content (plain, or stretched so that SAO clips at the ends of the sample range), its own SAO
depth and incoming disabled rates (both sides of the picture-level switch) -- against the oracle per slot, against the same picture run alone, and
for P / B slices against the reference's fixtures.  A slot that read its neighbour's descriptor would show here."""
import numpy as np
import pytest

import common
import synth

ZERO_POC = np.zeros((2, 16), np.int32)

# (QP, seed, stretched, SAO depth, incoming disabled rates [luma, cb, cr] at index depth - 1)
BATCHES = {
    "200x136_8b": (200, 136, 8, [(15, 2, False, 0, None), (16, 1, False, 0, None), (24, 1, False, 0, None),
                                 (24, 1, False, 1, (0.76, 0.49, 0.49)), (24, 1, False, 1, (0.75, 0.51, 0.51)),
                                 (24, 3, True, 0, None), (51, 3, False, 0, None)]),
    "136x72_10b": (136, 72, 10, [(15, 1, True, 0, None), (16, 1, True, 0, None), (24, 3, True, 0, None), (16, 3, False, 0, None), (45, 8, False, 0, None)]),
}


def stretch(planes, bd):
    """every plane mapped by clip((p - 2^(bd-1)) * 3 + 2^(bd-1), 0, 2^bd - 1): flat areas at both ends of the sample range"""
    half, top = 1 << (bd - 1), (1 << bd) - 1
    return [np.clip((p.astype(np.int32) - half) * 3 + half, 0, top).astype(np.uint16) for p in planes]


def incoming_rate(depth, rate_in):
    rate = np.zeros((3, 8), np.float64)
    if rate_in is not None:
        rate[:, depth - 1] = rate_in
    return rate


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


@pytest.fixture(scope="module")
def want(built, hm):
    """the oracle's search, deblocking, SAO and slice data of every slot of both batches; computed once, read-only"""
    import oracle
    out = {}
    for key, (w, h, bd, slots) in BATCHES.items():
        res = []
        for qp, seed, stretched, depth, rate_in in slots:
            planes = synth.frame(w, h, bd, 0, seed)
            if stretched:
                planes = stretch(planes, bd)
            lam, cw = hm.intra_lambda(qp)
            rec, ctus = oracle.compress(planes, bd, qp, 0)
            dbk = oracle.deblock(rec, bd, qp, 2, ZERO_POC, ctus, None)
            rate = incoming_rate(depth, rate_in)
            fin, params, en = oracle.sao(planes, dbk, bd, qp, lam, cw, 2, depth, rate)
            en = tuple(int(v) for v in en)
            subs, nxt, bins = oracle.encode_slice(w, h, bd, 0, 2, qp, ctus, sao=params, sao_enabled=en[:2])
            res.append(dict(qp=qp, planes=planes, lam=lam, cw=cw, depth=depth, rate_in=incoming_rate(depth, rate_in), rec=rec, ctus=ctus, dbk=dbk, fin=fin,
                            params=common.normalise_sao(params), en=en, rate_out=rate, bits=(subs, nxt, bins), stretched=stretched))
        out[key] = res
    return out


def _changed(a, b):
    return [int((a[c] != b[c]).sum()) for c in range(3)]


def test_oracle_results_of_the_batches_reach_the_edges(want):
    """what the slots are there for, asserted on the oracle's own results (no GPU), so that the comparisons below cannot pass emptily"""
    b8, b10 = want["200x136_8b"], want["136x72_10b"]
    for r in b8 + b10:
        ch = _changed(r["rec"], r["dbk"])
        if r["qp"] == 15:
            assert ch == [0, 0, 0], "beta == 0 below QP 16: deblocking changes nothing"
        if r["qp"] == 16:
            assert all(v > 0 for v in ch), f"QP 16: deblocking changes all three planes, {ch}"
        if r["qp"] >= 45:                         # the end of the tc table: no new offsets, more than 1,000 deblocked luma samples
            assert not (r["params"][:, :, 0] == 1).any() and ch[0] > 1000, (r["qp"], ch)
    # the picture-level switch: luma off above 0.75, chroma off above 0.5, on both sides of each threshold
    assert [r["en"] for r in b8 if r["depth"] == 1] == [(0, 1, 1), (1, 0, 0)]
    new8 = np.concatenate([r["params"].reshape(-1, 35)[r["params"].reshape(-1, 35)[:, 0] == 1] for r in b8])
    assert len(set(int(t) for t in new8[:, 1] if t < 4)) >= 3 and (new8[:, 1] == 4).any(), "edge-offset classes and the band offset among the new offsets"
    merges = np.concatenate([r["params"].reshape(-1, 35)[r["params"].reshape(-1, 35)[:, 0] == 2] for r in b8 + b10])
    assert (merges[:, 1] == 0).any() and (merges[:, 1] == 1).any(), "merge-left and merge-up"
    # SAO's clip at both ends of the sample range
    band = False
    for r, top in [(x, 255) for x in b8 if x["stretched"]] + [(x, 1023) for x in b10 if x["stretched"]]:
        moved = (r["fin"][0] != r["dbk"][0]) & ((r["fin"][0] == 0) | (r["fin"][0] == top))
        assert int(moved.sum()) > 30, f"QP {r['qp']}: SAO moved {int(moved.sum())} luma samples onto 0 or {top}"
        if top == 1023:
            new = r["params"].reshape(-1, 35)
            band = band or bool(((new[:, 0] == 1) & (new[:, 1] == 4)).any())
    assert band, "a stretched 10-bit slot with a band offset"


def _run_i_batch(hm, w, h, bd, slots):
    """slots (oracle results of `want`) through one launch per stage; -> per slot dict of what the device left after each stage"""
    n = len(slots)
    enc = hm.Encoder(w, h, bd, 0, max_batch=n)
    for k, r in enumerate(slots):
        enc.upload(k, r["planes"])
    sl = (hm.SliceDesc * n)(*[hm.SliceDesc(2, r["qp"], r["lam"], r["cw"]) for r in slots])
    enc._check(enc.lib.hm355_run(enc.h_, n, sl), "hm355_run")
    got = [dict(zip(("rec", "ctus"), enc.download(k)[:2])) for k in range(n)]
    enc.deblock_run([(2, r["qp"], None) for r in slots])
    for k in range(n):
        got[k]["dbk"] = enc.download(k, want_ctus=False)[0]
    descs = [dict(qp=r["qp"], cabac_init_type=2, depth=r["depth"], disabled_rate=r["rate_in"].copy(), chroma_weight=r["cw"], **{"lambda": r["lam"]}) for r in slots]
    sao = enc.sao_run(descs)
    for k in range(n):
        got[k]["fin"] = enc.download(k, want_ctus=False)[0]
        got[k]["en"], got[k]["params"] = sao[k][0], common.normalise_sao(sao[k][1])
        got[k]["rate_out"] = descs[k]["disabled_rate"]
    bits = enc.encode_slices_run([dict(slice_type=2, qp=r["qp"], sao_enabled=got[k]["en"][:2]) for k, r in enumerate(slots)])
    for k in range(n):
        got[k]["bits"] = bits[k]
    enc.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(BATCHES))
def test_hip_loop_filter_batch_with_a_descriptor_per_slot_matches_oracle(hm, want, key):
    """I pictures with a different QP, content, SAO depth and incoming disabled rates per slot: hm355_run, hm355_deblock_run, hm355_sao_run and
    hm355_encode_slices_run once each over the whole batch; after every stage every slot equals the oracle (search result, deblocked planes, SAO
    output planes, normalised parameters, enable flags, updated rates, substreams, bins, next table), and equals the same picture run alone in a
    one-slot encoder."""
    w, h, bd, _ = BATCHES[key]
    slots = want[key]
    got = _run_i_batch(hm, w, h, bd, slots)
    for k, (g, r) in enumerate(zip(got, slots)):
        what = f"{key} slot {k} (QP {r['qp']})"
        common.assert_ctus_equal(g["ctus"], r["ctus"], what)
        for stage in ("rec", "dbk", "fin"):
            for c in range(3):
                assert np.array_equal(g[stage][c], r[stage][c]), f"{what}: {stage} plane {c} differs at {int((g[stage][c] != r[stage][c]).sum())} samples"
        assert g["en"] == r["en"], f"{what}: SAO enable flags {g['en']} vs {r['en']}"
        assert np.array_equal(g["params"], r["params"]), f"{what}: SAO parameters"
        assert np.array_equal(np.asarray(g["rate_out"]), r["rate_out"]), f"{what}: updated disabled rates"
        assert g["bits"][0] == r["bits"][0] and g["bits"][1:] == r["bits"][1:], f"{what}: slice data"
    for k, r in enumerate(slots):
        alone, = _run_i_batch(hm, w, h, bd, [r])
        g, what = got[k], f"{key} slot {k} (QP {r['qp']}) vs the picture alone"
        assert g["ctus"].tobytes() == alone["ctus"].tobytes(), f"{what}: search result"
        for stage in ("rec", "dbk", "fin"):
            for c in range(3):
                assert np.array_equal(g[stage][c], alone[stage][c]), f"{what}: {stage} plane {c}"
        assert g["en"] == alone["en"] and np.array_equal(g["params"], alone["params"]), f"{what}: SAO decisions"
        assert np.array_equal(np.asarray(g["rate_out"]), np.asarray(alone["rate_out"])) and g["bits"] == alone["bits"], f"{what}: rates / slice data"


@pytest.mark.gpu
@pytest.mark.parametrize("name,slice_type", [("edge_ldp_136x72_8b_qp13", 1), ("edge_ldb_200x136_10b_qp46", 0)])
def test_hip_inter_loop_filter_batch_matches_reference(built, hm, name, slice_type):
    """The three P slices of the clip around QP 16 (16, 15, 16: in one launch the deblocking filter is off for the picture in the middle and on for
    its neighbours) and the three B slices of the 10-bit QP-46 clip: one hm355_compress_slices_inter with the references from the fixture's
    finished pictures, then hm355_deblock_run, hm355_sao_run and hm355_encode_slices_run with three descriptors.  Finished pictures, SAO parameters,
    flags and substreams equal the reference's fixture.  The disabled rates each picture comes in with are those of the oracle's SAO replayed over
    the clip on the CPU (the chain test_oracle_deblocking_and_sao_match_reference_at_the_edges pins to the fixture)."""
    import oracle
    saod, bitd = {}, {}
    cfg, slices, finals = common.load_ldp_case(name, sao=saod, bits=bitd)
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    rate, rates_in, rates_out = np.zeros((3, 8), np.float64), {}, {}
    for r in slices:
        poc = int(r["poc"])
        rates_in[poc] = rate.copy()
        ctus, ictus = common.split_fixture_ctus(r["ctus"])
        dbk = oracle.deblock(r["rec"], bd, int(r["qp"]), int(r["slice_type"]), r["ref_poc"], ctus, ictus)
        oracle.sao(synth.frame(w, h, bd, poc, cfg["seed"]), dbk, bd, int(r["qp"]), float(r["lambda"]), float(r["weight_cb"]), int(r["cabac_init_type"]),
                   saod[poc]["depth"], rate)
        rates_out[poc] = rate.copy()
    ps = [r for r in slices if int(r["slice_type"]) == slice_type]
    assert len(ps) == 3 and len(slices) == 4
    if name.endswith("qp13"):
        assert [int(r["qp"]) for r in ps] == [16, 15, 16]
    enc = hm.Encoder(w, h, bd, cfg["wpp"], max_batch=3)
    jobs = []
    for r in ps:
        sp, refs = common.ldp_slice_inputs(r, finals)
        jobs.append((synth.frame(w, h, bd, int(r["poc"]), cfg["seed"]), sp, refs))
    for r, (rec, ctus, ictus, _) in zip(ps, enc.compress_inter_batch(jobs)):
        common.assert_inter_ctus_equal(ctus, ictus, r["ctus"], f"{name} POC {int(r['poc'])}")
        for c in range(3):
            assert np.array_equal(rec[c], r["rec"][c]), f"{name} POC {int(r['poc'])}: reconstruction plane {c}"
    enc.deblock_run([(slice_type, int(r["qp"]), r["ref_poc"]) for r in ps])
    sao = enc.sao_run([dict(qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), depth=saod[int(r["poc"])]["depth"], disabled_rate=rates_in[int(r["poc"])],
                            chroma_weight=float(r["weight_cb"]), **{"lambda": float(r["lambda"])}) for r in ps])
    bits = enc.encode_slices_run([dict(slice_type=slice_type, qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), num_ref_idx=r["num_ref_idx"],
                                       mvd_l1_zero=int(r["mvd_l1_zero"]), max_merge_cand=int(r["max_merge_cand"]), sao_enabled=sao[k][0][:2]) for k, r in enumerate(ps)])
    for k, r in enumerate(ps):
        poc = int(r["poc"])
        a, what = saod[poc], f"{name} POC {poc} (slot {k})"
        en, params = sao[k]
        assert (en[0], en[1]) == tuple(a["enabled"]) and en[1] == en[2], f"{what}: slice-level SAO flags {en} vs {a['enabled']}"
        assert np.array_equal(common.normalise_sao(params), common.normalise_sao(a["sao"])), f"{what}: SAO parameters"
        assert np.array_equal(rates_in[poc], rates_out[poc]), f"{what}: updated disabled rates"          # sao_run updated rates_in[poc] in place
        fin = enc.download(k, want_ctus=False)[0]
        for c in range(3):
            assert np.array_equal(fin[c], finals[poc]["rec"][c]), f"{what}: finished picture plane {c} differs at {int((fin[c] != finals[poc]['rec'][c]).sum())} samples"
        subs, nxt, bins = bits[k]
        assert subs == bitd[poc]["substreams"], f"{what}: slice data bytes differ"
        assert (nxt, bins) == (bitd[poc]["next_cabac_init_type"], bitd[poc]["num_bins"]), f"{what}: next context table / bin count"
    enc.close()
