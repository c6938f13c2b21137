"""GPU suite (-m gpu): tiles (hm355_set_tiles) -- tile-scan search with tile-restricted neighbours, SAO merge candidates inside the tile, one
substream per tile -- against clips the real reference encoded with tiles (tests/gen_golden_tiles.py)."""
import os
import subprocess

import numpy as np
import pytest

import common
import synth
from test_tiles_host import TILE_CASES, fixture_layout

pytestmark = pytest.mark.gpu
UNTILED = "ldp2gop_256x128_8b_qp34"         # 4 x 2 CTUs: wide enough for a tile layout of its own (one column, two rows)


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


def _frame(cfg, poc):
    return synth.frame(cfg["width"], cfg["height"], cfg["bit_depth"], int(poc), cfg["seed"])


def _encoder(hm, cfg, name=None, max_batch=1):
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=max_batch)
    if name:
        cols, rows, _ = fixture_layout(name)
        enc.set_tiles(cols, rows)
    return enc


def _search(hm, enc, cfg, r, finals, refs=None):
    """one slice of a fixture through the search -> (rec, ctus, ictus or None); compares nothing"""
    planes = _frame(cfg, r["poc"])
    if int(r["slice_type"]) == 2:
        enc.upload(0, planes)
        sl = (hm.SliceDesc * 1)(hm.SliceDesc(2, int(r["qp"]), float(r["lambda"]), float(r["weight_cb"])))
        enc._check(enc.lib.hm355_run(enc.h_, 1, sl), "hm355_run")
        rec, ctus, _ = enc.download(0)
        return rec, ctus, None
    sp, refs = common.ldp_slice_inputs(r, finals, refs)
    rec, ctus, ictus, _ = enc.compress_inter(planes, sp, refs)
    return rec, ctus, ictus


def _assert_slice(got, r, what):
    rec, ctus, ictus = got
    if ictus is None:
        common.assert_ctus_equal(ctus, common.split_fixture_ctus(r["ctus"])[0], what)
    else:
        common.assert_inter_ctus_equal(ctus, ictus, r["ctus"], what)
    for c in range(3):
        assert np.array_equal(rec[c], r["rec"][c]), f"{what}: reconstruction plane {c}"


def _want_shape(n_ctus, tiles, inter, team, pictures=1, max_batch=1):
    """hm355_plan_launch for a tiled launch without WaveFrontSynchro on an otherwise idle context (every team gets its windows)"""
    total = pictures * n_ctus
    ws = min(max(n_ctus * max_batch * 9, 12), 3072)
    if team:
        waves = 9 if inter else 5
        return dict(kernel="team", waves=waves, few_waves=1, workgroups=min(pictures * tiles + 2, total, 512, ws // waves), tickets=total)
    groups = min((min(total, ws) + 11) // 12, ws // 12)
    return dict(kernel="search12", waves=12, few_waves=1, workgroups=groups, tickets=total)


@pytest.mark.parametrize("team", ["0", "1"])
@pytest.mark.parametrize("name", TILE_CASES)
def test_hip_tiled_search_matches_reference_fixture(hm, monkeypatch, name, team):
    """every slice of the four clips through the search with the fixture's tile layout, as teams of wavefronts and with one wavefront per CTU:
    every field of every CTU and the reconstruction, and the launch shape the plan gives for `tiles` chains per picture"""
    monkeypatch.setenv("HM355_TEAM", team)
    cfg, slices, finals = common.load_ldp_case(name)
    cols, rows, _ = fixture_layout(name)
    enc = _encoder(hm, cfg, name)
    assert enc.lib.hm355_num_substreams(enc.h_) == len(cols) * len(rows)
    for r in slices:
        _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{name} POC {int(r['poc'])} HM355_TEAM={team}")
        assert enc.last_launch_shape() == _want_shape(enc.num_ctus, len(cols) * len(rows), int(r["slice_type"]) != 2, team == "1")
    enc.close()


@pytest.mark.parametrize("name", TILE_CASES)
def test_hip_tiled_closed_loop_on_device_matches_reference(hm, name):
    """search -> hm355_deblock_run -> hm355_sao_run -> hm355_encode_slices_run -> hm355_ref_from_slot -> the next picture in coding order, all with
    the fixture's tiles: the finished pictures ('F'), the SAO parameters and slice flags ('A'), and the bytes of the rows x cols substreams, the
    bin count and the next context table ('B')"""
    saod, bitd = {}, {}
    cfg, slices, finals = common.load_ldp_case(name, sao=saod, bits=bitd)
    cols, rows, _ = fixture_layout(name)
    rate = np.zeros((3, 8), np.float64)
    enc = _encoder(hm, cfg, name)
    dev_refs = {}
    for r in slices:
        st, poc = int(r["slice_type"]), int(r["poc"])
        refs = {int(p): dev_refs[int(p)] for l in range(2) for p in r["ref_poc"][l][:r["num_ref_idx"][l]]} if st != 2 else None
        _assert_slice(_search(hm, enc, cfg, r, finals, refs), r, f"{name} POC {poc} (device-resident references)")
        assert enc.last_launch_shape()["tickets"] == enc.num_ctus and enc.last_launch_shape()["kernel"] == "team"
        enc.deblock_run([(st, int(r["qp"]), r["ref_poc"])])
        a = saod[poc]
        (en, params), = enc.sao_run([dict(qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), depth=a["depth"], disabled_rate=rate,
                                          chroma_weight=float(r["weight_cb"]), **{"lambda": float(r["lambda"])})])
        assert (en[0], en[1]) == tuple(a["enabled"]) and en[1] == en[2], f"{name} POC {poc}: slice-level SAO flags {en} vs {a['enabled']}"
        assert np.array_equal(common.normalise_sao(params), common.normalise_sao(a["sao"])), f"{name} POC {poc}: SAO parameters"
        (subs, nxt, bins), = enc.encode_slices_run([dict(slice_type=st, qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), num_ref_idx=r["num_ref_idx"],
                                                         mvd_l1_zero=int(r["mvd_l1_zero"]), max_merge_cand=int(r["max_merge_cand"]), sao_enabled=(en[0], en[1]))])
        assert len(subs) == len(cols) * len(rows)
        assert subs == bitd[poc]["substreams"], f"{name} POC {poc}: slice data bytes differ in substreams {[k for k in range(len(subs)) if subs[k] != bitd[poc]['substreams'][k]]}"
        assert (nxt, bins) == (bitd[poc]["next_cabac_init_type"], bitd[poc]["num_bins"]), f"{name} POC {poc}: next context table / bin count"
        out, _, _ = enc.download(0, want_ctus=False)
        for c in range(3):
            assert np.array_equal(out[c], finals[poc]["rec"][c]), f"{name} POC {poc}: finished picture plane {c}"
        dev_refs[poc] = enc.ref_from_slot(0, poc, st != 2, r["num_ref_idx"], r["ref_poc"], r["ref_long_term"])
    for ref in dev_refs.values():
        enc.ref_release(ref)
    enc.close()


def test_hip_tiled_batch_of_80_runs_as_160_chains(hm):
    """the first picture of the all-intra 2 x 1 clip in 80 slots of one hm355_run: 160 independent chains, so the plan asks for 162 teams of five
    wavefronts; every slot equals the fixture"""
    name = TILE_CASES[0]
    cfg, slices, finals = common.load_ldp_case(name)
    r = slices[0]
    n = 80
    enc = _encoder(hm, cfg, name, max_batch=n)
    planes = _frame(cfg, r["poc"])
    for s in range(n):
        enc.upload(s, planes)
    sl = (hm.SliceDesc * n)(*[hm.SliceDesc(2, int(r["qp"]), float(r["lambda"]), float(r["weight_cb"])) for _ in range(n)])
    enc._check(enc.lib.hm355_run(enc.h_, n, sl), "hm355_run")
    assert enc.last_launch_shape() == _want_shape(enc.num_ctus, 2, False, True, pictures=n, max_batch=n) == dict(kernel="team", waves=5, few_waves=1, workgroups=162, tickets=n * 27)
    for s in range(n):
        rec, ctus, _ = enc.download(s)
        _assert_slice((rec, ctus, None), r, f"{name} slot {s}")
    enc.close()


def _pipeline(enc, recs, saod, rates):
    """hm355_deblock_run, hm355_sao_run and hm355_encode_slices_run once over slots 0..len(recs)-1, every slot with the descriptor of its own
    'S' record and its own SAO disabled-rate table (updated in place) -> per slot (finished picture, SAO flags, SAO parameters, substreams, next
    context table, bins)"""
    enc.deblock_run([(int(r["slice_type"]), int(r["qp"]), r["ref_poc"]) for r in recs])
    sao = enc.sao_run([dict(qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), depth=saod[int(r["poc"])]["depth"], disabled_rate=rate,
                            chroma_weight=float(r["weight_cb"]), **{"lambda": float(r["lambda"])}) for r, rate in zip(recs, rates)])
    bits = enc.encode_slices_run([dict(slice_type=int(r["slice_type"]), qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), num_ref_idx=r["num_ref_idx"],
                                       mvd_l1_zero=int(r["mvd_l1_zero"]), max_merge_cand=int(r["max_merge_cand"]), sao_enabled=(en[0], en[1])) for r, (en, _) in zip(recs, sao)])
    return [(enc.download(s, want_ctus=False)[0], sao[s][0], sao[s][1]) + bits[s] for s in range(len(recs))]


def test_hip_tiled_batch_of_different_pictures_through_the_pipeline(hm):
    """a DIFFERENT picture in every slot of a tiled launch, and of the loop filter and bitstream passes behind it: the two I pictures of the
    all-intra 2 x 1 clip in slots 0 and 1 of one hm355_run; the three P slices of the low-delay 2 x 2 clip in one hm355_compress_slices_inter
    call (references: the fixture's finished pictures), which leaves its results resident in slots 0..2.  Then one hm355_deblock_run, one
    hm355_sao_run and one hm355_encode_slices_run over all slots.  Every slot's CTUs, finished picture, SAO parameters and substreams equal its
    own 'S' / 'F' / 'A' / 'B' records -- a launch that read another slot's neighbour, hand-off state or tile table entry would not -- and
    equal the same picture taken through the same calls alone on a context of one slot.
    The pictures alone come first, the whole clip in coding order: SAO's m_saoDisabledRate runs from picture to picture (POC 2 of the low-delay
    clip, depth 1, has chroma SAO off because of the I picture's rate), so every slot of the batch is handed the table as it stood before its
    picture."""
    for name, pick in ((TILE_CASES[0], lambda r: True), (TILE_CASES[2], lambda r: int(r["slice_type"]) == 1)):
        saod, bitd = {}, {}
        cfg, slices, finals = common.load_ldp_case(name, sao=saod, bits=bitd)
        cols, rows, _ = fixture_layout(name)
        recs = [r for r in slices if pick(r)]
        n, inter = len(recs), int(recs[0]["slice_type"]) != 2
        assert n == (3 if inter else 2) and len(set(int(r["poc"]) for r in recs)) == n

        def search(enc, some):
            if int(some[0]["slice_type"]) != 2:
                out = enc.compress_inter_batch([(_frame(cfg, r["poc"]),) + common.ldp_slice_inputs(r, finals) for r in some])
                return [(o[0], o[1], o[2]) for o in out]
            for s, r in enumerate(some):
                enc.upload(s, _frame(cfg, r["poc"]))
            sl = (hm.SliceDesc * len(some))(*[hm.SliceDesc(2, int(r["qp"]), float(r["lambda"]), float(r["weight_cb"])) for r in some])
            enc._check(enc.lib.hm355_run(enc.h_, len(some), sl), "hm355_run")
            return [enc.download(s)[:2] + (None,) for s in range(len(some))]

        alone, rate, rate_before, single = _encoder(hm, cfg, name), np.zeros((3, 8), np.float64), {}, {}
        for r in slices:
            rate_before[int(r["poc"])] = rate.copy()
            one, = search(alone, [r])
            single[int(r["poc"])] = (one,) + _pipeline(alone, [r], saod, [rate])[0]
        alone.close()
        assert not inter or any(rate_before[int(r["poc"])].any() for r in recs), "the rate table should matter to a slot"
        enc = _encoder(hm, cfg, name, max_batch=n)
        got = search(enc, recs)
        shape = enc.last_launch_shape()
        assert shape["tickets"] == n * enc.num_ctus and shape == _want_shape(enc.num_ctus, len(cols) * len(rows), inter, True, pictures=n, max_batch=n), shape
        piped = _pipeline(enc, recs, saod, [rate_before[int(r["poc"])].copy() for r in recs])
        enc.close()
        for s, r in enumerate(recs):
            poc, what = int(r["poc"]), f"{name} POC {int(r['poc'])} in slot {s} of {n}"
            _assert_slice(got[s], r, what)
            fin, en, params, subs, nxt, bins = piped[s]
            assert (en[0], en[1]) == tuple(saod[poc]["enabled"]), f"{what}: slice-level SAO flags {en} vs {saod[poc]['enabled']}"
            assert np.array_equal(common.normalise_sao(params), common.normalise_sao(saod[poc]["sao"])), f"{what}: SAO parameters"
            for c in range(3):
                assert np.array_equal(fin[c], finals[poc]["rec"][c]), f"{what}: finished picture plane {c}"
            assert subs == bitd[poc]["substreams"] and len(subs) == len(cols) * len(rows), f"{what}: slice data bytes"
            assert (nxt, bins) == (bitd[poc]["next_cabac_init_type"], bitd[poc]["num_bins"]), f"{what}: next context table / bin count"
            one, afin, aen, aparams, asubs, anxt, abins = single[poc]
            for k in (1, 2):
                if one[k] is not None:
                    for f in one[k].dtype.names:
                        assert np.array_equal(one[k][f], got[s][k][f]), f"{what}: {f} differs from the picture searched alone"
            assert all(np.array_equal(one[0][c], got[s][0][c]) and np.array_equal(afin[c], fin[c]) for c in range(3)), f"{what}: planes differ from the picture alone"
            assert aen == en and np.array_equal(common.normalise_sao(aparams), common.normalise_sao(params)) and (asubs, anxt, abins) == (subs, nxt, bins), f"{what}: SAO / slice data differ from the picture alone"


@pytest.mark.parametrize("name,mode,tiles", [(TILE_CASES[2], "ldp", "tiles=2x2"), (TILE_CASES[1], "lf", "tiles=c:4,4,5;r:1,1")])
def test_cpp_host_mirror_with_tiles(tmp_path, name, mode, tiles):
    """hm355_encmain tiles=...: from the raw YUV through search, loop filters, slice data and device-resident references; every substream of
    every picture byte for byte as the reference wrote it with the same tiles"""
    bd = {}
    cfg, slices, _ = common.load_ldp_case(name, bits=bd)
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump.bin"
    synth.write_yuv(str(yuv), cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["seed"])
    exe = os.path.join(common.ROOT, "hm-16.2_amd", "hm355_encmain")
    subprocess.run([exe, str(yuv), str(cfg["width"]), str(cfg["height"]), str(cfg["bit_depth"]), str(cfg["frames"]), str(int(slices[0]["qp"])), "0",
                    str(dump), mode, tiles], check=True)
    bits = common.read_mirror_bits(str(dump) + ".bits", cfg["frames"])
    cols, rows, _ = fixture_layout(name)
    assert len(slices) == cfg["frames"]
    for i, r in enumerate(slices):
        assert len(bits[i]) == len(cols) * len(rows)
        assert bits[i] == bd[int(r["poc"])]["substreams"], f"{name} POC {int(r['poc'])}: slice data bytes"


def test_set_tiles_rejections_leave_the_layout_in_force(hm):
    """each refusal by its message; after all of them the search still reproduces the clip with the layout set before"""
    name = TILE_CASES[0]
    cfg, slices, finals = common.load_ldp_case(name)
    enc = _encoder(hm, cfg, name)
    for args, msg in ((((3, 6), (3,)), "narrower than 4 CTUs"), (((4, 4), (3,)), "column widths do not sum"), (((4, 5), (2,)), "row heights do not sum"),
                      (((4, 5), (3,), 0), "lf_cross_tile must be 1")):
        with pytest.raises(RuntimeError, match=msg):
            enc.set_tiles(*args)
    with pytest.raises(RuntimeError, match="hm355_set_dqp: not with tiles"):
        enc.set_dqp(0, None, 0)
    with pytest.raises(RuntimeError, match="hm355_run_rows: not with tiles"):
        enc.run_rows(0, 1, 30, 0, 0)
    enc.upload(0, _frame(cfg, 0))
    with pytest.raises(RuntimeError, match="hm355_slice_begin: not with tiles"):
        enc.slice_begin(0, 30, *hm.intra_lambda(30))
    assert enc.lib.hm355_num_substreams(enc.h_) == 2
    _assert_slice(_search(hm, enc, cfg, slices[0], finals), slices[0], f"{name} after the refused calls")
    enc.close()
    wpp = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], 1, max_batch=1)
    with pytest.raises(RuntimeError, match="WaveFrontSynchro"):
        wpp.set_tiles((4, 5), (3,))
    wpp.set_tiles()                                        # one tile is no tiles: allowed
    wpp.close()


def test_tiles_off_again_leaves_no_tile_state(hm):
    """a clip of the default configuration on a context that searched with tiles before: with hm355_set_tiles(1, ..., 1, ...) it equals its
    fixture, slice data included; with the tiles left on it does not"""
    bitd = {}
    cfg, slices, finals = common.load_ldp_case(UNTILED, bits=bitd)
    ps = [r for r in slices if int(r["slice_type"]) != 2][:2]
    enc = _encoder(hm, cfg)
    enc.set_tiles((4,), (1, 1))
    assert enc.lib.hm355_num_substreams(enc.h_) == 2
    with pytest.raises(AssertionError):
        _assert_slice(_search(hm, enc, cfg, ps[0], finals), ps[0], "tiled")
    enc.set_tiles((4,), (2,))
    assert enc.lib.hm355_num_substreams(enc.h_) == 1
    for r in ps:
        _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{UNTILED} POC {int(r['poc'])} after tiles")
        assert enc.last_launch_shape()["tickets"] == enc.num_ctus
    r = slices[0]                                          # the I picture through the whole pipeline: one substream, SAO merge candidates across the former tile edge
    _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{UNTILED} POC 0 after tiles")
    saod = {}
    common.load_ldp_case(UNTILED, sao=saod)
    rate = np.zeros((3, 8), np.float64)
    enc.deblock_run([(2, int(r["qp"]), r["ref_poc"])])
    (en, _), = enc.sao_run([dict(qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), depth=saod[0]["depth"], disabled_rate=rate,
                                 chroma_weight=float(r["weight_cb"]), **{"lambda": float(r["lambda"])})])
    (subs, nxt, bins), = enc.encode_slices_run([dict(slice_type=2, qp=int(r["qp"]), sao_enabled=(en[0], en[1]))])
    assert subs == bitd[0]["substreams"] and bins == bitd[0]["num_bins"]
    enc.close()
