"""GPU suite (-m gpu): slices (hm355_set_slices) -- one chain of CTU searches per slice with slice-restricted neighbours, SAO merge candidates
inside the slice, one substream per slice with the context table chained from slice to slice -- against clips the real reference encoded with
--SliceMode=1 (tests/gen_golden_slices.py)."""
import os
import subprocess

import numpy as np
import pytest

import common
import synth
from slices_common import SLICE_CASES, load_slices_case
from test_gpu_tiles import _assert_slice, _frame, _search, _want_shape

pytestmark = pytest.mark.gpu
UNSLICED = "ldp2gop_256x128_8b_qp34"


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


def _encoder(hm, cfg, first=None, max_batch=1):
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=max_batch)
    if first is not None:
        enc.set_slices(first)
    return enc


@pytest.mark.parametrize("team", ["0", "1"])
@pytest.mark.parametrize("name", SLICE_CASES)
def test_hip_sliced_search_matches_reference_fixture(hm, monkeypatch, name, team):
    """every picture of the clips through the search with the fixture's partition, as teams of wavefronts and with one wavefront per CTU: every
    field of every CTU and the reconstruction, and the launch shape the plan gives for `slices` chains per picture"""
    monkeypatch.setenv("HM355_TEAM", team)
    cfg, slices, finals, _, _, extra = load_slices_case(name)
    first = extra["slice_first_ctu"]
    enc = _encoder(hm, cfg, first)
    assert enc.lib.hm355_num_substreams(enc.h_) == enc.lib.hm355_num_slices(enc.h_) == len(first)
    assert list(hm.fixed_ctu_slices(enc.lib, (cfg["width"] + 63) // 64, (cfg["height"] + 63) // 64, 0, int(extra["slice_arg"]))) == list(first)
    for r in slices:
        _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{name} POC {int(r['poc'])} HM355_TEAM={team}")
        assert enc.last_launch_shape() == _want_shape(enc.num_ctus, len(first), int(r["slice_type"]) != 2, team == "1")
    enc.close()


@pytest.mark.parametrize("name", SLICE_CASES)
def test_hip_sliced_closed_loop_on_device_matches_reference(hm, name):
    """search -> hm355_deblock_run -> hm355_sao_run -> hm355_encode_slices_run -> hm355_ref_from_slot -> the next picture in coding order: the
    finished pictures ('F'), the SAO parameters and slice flags ('A'), and per slice the substream bytes, the next context table and the bin
    count ('B') -- POC 1 of the random-access clip changes the table inside the picture"""
    cfg, slices, finals, saod, bitd, extra = load_slices_case(name)
    first = extra["slice_first_ctu"]
    rate = np.zeros((3, 8), np.float64)
    enc = _encoder(hm, cfg, first)
    dev_refs, changed = {}, 0
    for r in slices:
        st, poc = int(r["slice_type"]), int(r["poc"])
        refs = {int(p): dev_refs[int(p)] for l in range(2) for p in r["ref_poc"][l][:r["num_ref_idx"][l]]} if st != 2 else None
        _assert_slice(_search(hm, enc, cfg, r, finals, refs), r, f"{name} POC {poc} (device-resident references)")
        enc.deblock_run([(st, int(r["qp"]), r["ref_poc"])])
        a = saod[poc]
        (en, params), = enc.sao_run([dict(qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), depth=a["depth"], disabled_rate=rate,
                                          chroma_weight=float(r["weight_cb"]), **{"lambda": float(r["lambda"])})])
        assert (en[0], en[1]) == tuple(a["enabled"]) and en[1] == en[2], f"{name} POC {poc}: slice-level SAO flags {en} vs {a['enabled']}"
        assert np.array_equal(common.normalise_sao(params), common.normalise_sao(a["sao"])), f"{name} POC {poc}: SAO parameters"
        (subs, nxt, bins), = enc.encode_slices_run([dict(slice_type=st, qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), num_ref_idx=r["num_ref_idx"],
                                                         mvd_l1_zero=int(r["mvd_l1_zero"]), max_merge_cand=int(r["max_merge_cand"]), sao_enabled=(en[0], en[1]))])
        want = bitd[poc]
        assert len(subs) == len(want) == len(first)
        for k, b in enumerate(want):
            assert [subs[k]] == [s for s in b["substreams"] if len(s)], f"{name} POC {poc} slice {k}: slice data bytes"
        info = enc.slice_bits_info(0)
        assert info == [(1, b["next_cabac_init_type"], b["num_bins"]) for b in want], f"{name} POC {poc}: per-slice next table / bins {info}"
        assert (nxt, bins) == (want[-1]["next_cabac_init_type"], sum(b["num_bins"] for b in want))
        changed += st != 2 and any(b["next_cabac_init_type"] != int(r["cabac_init_type"]) for b in want[:-1])
        out, _, _ = enc.download(0, want_ctus=False)
        for c in range(3):
            assert np.array_equal(out[c], finals[poc]["rec"][c]), f"{name} POC {poc}: finished picture plane {c}"
        dev_refs[poc] = enc.ref_from_slot(0, poc, st != 2, r["num_ref_idx"], r["ref_poc"], r["ref_long_term"])
    if name == SLICE_CASES[2]:
        assert changed >= 1, "the random-access clip should change the context table inside a picture"
    for ref in dev_refs.values():
        enc.ref_release(ref)
    enc.close()


def test_hip_sliced_batch_of_40_runs_as_120_chains(hm):
    """the intra clip in 40 slots of one hm355_run: 120 independent chains; every slot equals the fixture"""
    name = SLICE_CASES[0]
    cfg, slices, finals, _, _, extra = load_slices_case(name)
    r, n = slices[0], 40
    enc = _encoder(hm, cfg, extra["slice_first_ctu"], max_batch=n)
    planes = _frame(cfg, r["poc"])
    for s in range(n):
        enc.upload(s, planes)
    sl = (hm.SliceDesc * n)(*[hm.SliceDesc(2, int(r["qp"]), float(r["lambda"]), float(r["weight_cb"])) for _ in range(n)])
    enc._check(enc.lib.hm355_run(enc.h_, n, sl), "hm355_run")
    assert enc.last_launch_shape() == _want_shape(enc.num_ctus, 3, False, True, pictures=n, max_batch=n) == dict(kernel="team", waves=5, few_waves=1, workgroups=122, tickets=n * 24)
    for s in range(n):
        rec, ctus, _ = enc.download(s)
        _assert_slice((rec, ctus, None), r, f"{name} slot {s}")
    enc.close()


def test_two_slots_with_different_qps_in_one_bitstream_pass(hm):
    """the intra clip's picture searched at the fixture's QP in slot 0 and two steps above it in slot 1, both through one hm355_encode_slices_run
    (no SAO syntax, so the 'B' records do not apply): each slot, bytes and per-slice values, equals the same CTU data coded alone"""
    name = SLICE_CASES[0]
    cfg, slices, finals, _, bitd, extra = load_slices_case(name)
    r = slices[0]
    qps = [int(r["qp"]), int(r["qp"]) + 2]
    enc = _encoder(hm, cfg, extra["slice_first_ctu"], max_batch=2)
    planes = _frame(cfg, r["poc"])
    for s in range(2):
        enc.upload(s, planes)
    sl = (hm.SliceDesc * 2)(hm.SliceDesc(2, qps[0], float(r["lambda"]), float(r["weight_cb"])), hm.SliceDesc(2, qps[1], *hm.intra_lambda(qps[1])))
    enc._check(enc.lib.hm355_run(enc.h_, 2, sl), "hm355_run")
    both = enc.encode_slices_run([dict(slice_type=2, qp=q) for q in qps])
    infos = [enc.slice_bits_info(s) for s in range(2)]
    assert both[0][0] != both[1][0]
    assert len(both[0][0]) == len(both[1][0]) == 3 and all(i[1] == 2 for info in infos for i in info)
    alone = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], 0, max_batch=1)
    alone.set_slices(extra["slice_first_ctu"])
    for s in range(2):
        assert alone.encode_slice(dict(slice_type=2, qp=qps[s]), enc.download(s)[1]) == both[s], f"slot {s}"
        assert alone.slice_bits_info(0) == infos[s] and sum(i[2] for i in infos[s]) == both[s][2]
    alone.close()
    enc.close()


def test_two_slots_of_b_pictures_chain_their_tables_in_one_bitstream_pass(hm):
    """two B pictures of the random-access clip (POC 1, whose slices change the context table, and another) in two slots of one
    hm355_encode_slices_run: the tickets of the two pictures interleave, slice k of each waits for slice k - 1 of the same picture.  Without SAO
    syntax (the 'B' records carry it), so each slot is held against the same CTU data coded alone, the path the closed-loop test holds against the
    'B' records"""
    name = SLICE_CASES[2]
    cfg, slices, finals, _, _, extra = load_slices_case(name)
    inter = [r for r in slices if int(r["slice_type"]) != 2]
    pair = [[r for r in inter if int(r["poc"]) == 1][0], [r for r in inter if int(r["poc"]) != 1][0]]
    enc = _encoder(hm, cfg, extra["slice_first_ctu"], max_batch=2)
    jobs = []
    for r in pair:
        sp, refs = common.ldp_slice_inputs(r, finals)
        jobs.append((_frame(cfg, r["poc"]), sp, refs))
    out = enc.compress_inter_batch(jobs)
    for s, r in enumerate(pair):
        common.assert_inter_ctus_equal(out[s][1], out[s][2], r["ctus"], f"{name} POC {int(r['poc'])} in slot {s}")
    descs = [dict(slice_type=int(r["slice_type"]), qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), num_ref_idx=r["num_ref_idx"],
                  mvd_l1_zero=int(r["mvd_l1_zero"]), max_merge_cand=int(r["max_merge_cand"])) for r in pair]
    both = enc.encode_slices_run(descs)
    infos = [enc.slice_bits_info(s) for s in range(2)]
    assert both[0][0] != both[1][0] and all(len(b[0]) == 3 for b in both)
    alone = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], 0, max_batch=1)
    alone.set_slices(extra["slice_first_ctu"])
    for s in range(2):
        assert alone.encode_slice(descs[s], out[s][1], out[s][2]) == both[s], f"slot {s}"
        assert alone.slice_bits_info(0) == infos[s] and infos[s][-1][1] == both[s][1] and sum(i[2] for i in infos[s]) == both[s][2]
    alone.close()
    enc.close()


def test_cpp_host_mirror_with_slices(tmp_path):
    """hm355_encmain slices=<N> on the low-delay clip: every slice of every picture byte for byte as the reference wrote it"""
    name = SLICE_CASES[1]
    cfg, slices, _, _, bitd, extra = load_slices_case(name)
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump.bin"
    synth.write_yuv(str(yuv), cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["seed"])
    exe = os.path.join(common.ROOT, "hm-16.2_amd", "hm355_encmain")
    subprocess.run([exe, str(yuv), str(cfg["width"]), str(cfg["height"]), str(cfg["bit_depth"]), str(cfg["frames"]), str(int(extra["qp"])), "0",
                    str(dump), "ldp", f"slices={int(extra['slice_arg'])}"], check=True)
    bits = common.read_mirror_bits(str(dump) + ".bits", cfg["frames"])
    assert len(slices) == cfg["frames"]
    for i, r in enumerate(slices):
        want = [s for b in bitd[int(r["poc"])] for s in b["substreams"] if len(s)]
        assert bits[i] == want, f"{name} POC {int(r['poc'])}: slice data bytes"


def test_set_slices_rejections_leave_the_partition_in_force(hm):
    """each refusal by its message; after all of them the search still reproduces the clip with the partition set before"""
    name = SLICE_CASES[0]
    cfg, slices, finals, _, _, extra = load_slices_case(name)
    first = [int(v) for v in extra["slice_first_ctu"]]
    enc = _encoder(hm, cfg, first)
    for args, msg in ((([1, 8],), "does not start at CTU 0"), (([0, 8, 8],), "not ascending"), (([0, 16, 8],), "not ascending"), (([0, 24],), "past the picture"),
                      (([0, 8], 0), "lf_cross_slice must be 1")):
        with pytest.raises(RuntimeError, match=msg):
            enc.set_slices(*args)
    with pytest.raises(RuntimeError, match="hm355_set_tiles: not with slices"):
        enc.set_tiles((6,), (2, 2))
    with pytest.raises(RuntimeError, match="hm355_set_dqp: not with slices"):
        enc.set_dqp(0, None, 0)
    with pytest.raises(RuntimeError, match="hm355_run_rows: not with slices"):
        enc.run_rows(0, 1, 30, 0, 0)
    enc.upload(0, _frame(cfg, 0))
    with pytest.raises(RuntimeError, match="hm355_slice_begin: not with slices"):
        enc.slice_begin(0, 30, *hm.intra_lambda(30))
    with pytest.raises(RuntimeError, match="hm355_run_ctus: not with slices"):
        enc.run_ctus(0, 1, 0, 1)
    with pytest.raises(RuntimeError, match="hm355_export_boundary / hm355_import_boundary: not with slices"):
        enc.export_boundary(0, 0)
    with pytest.raises(RuntimeError, match="hm355_export_boundary / hm355_import_boundary: not with slices"):
        enc.import_boundary(0, 0, np.zeros(enc.boundary_bytes(), np.uint8))
    pcfg, pslices, pfinals, _, _, _ = load_slices_case(SLICE_CASES[1])          # a well-formed P slice descriptor: the refusal comes before it is read
    sp, host_refs = common.ldp_slice_inputs([r for r in pslices if int(r["slice_type"]) != 2][0], pfinals)
    with pytest.raises(RuntimeError, match="hm355_slice_begin_inter: not with slices"):
        enc.slice_begin_inter(0, sp, host_refs)
    assert enc.lib.hm355_num_substreams(enc.h_) == enc.lib.hm355_num_slices(enc.h_) == 3
    _assert_slice(_search(hm, enc, cfg, slices[0], finals), slices[0], f"{name} after the refused calls")
    enc.close()
    # a slice open on a slot, cu_qp_delta armed on a slot, tiles in force
    enc = _encoder(hm, cfg)
    enc.upload(0, _frame(cfg, 0))
    enc.set_dqp(0, None, 0)                                # hm355_slice_begin needs the slot armed
    with pytest.raises(RuntimeError, match="cu_qp_delta"):
        enc.set_slices(first)
    enc.slice_begin(0, 30, *hm.intra_lambda(30))
    with pytest.raises(RuntimeError, match="a slice is open"):
        enc.set_slices(first)
    enc.slice_end(0)
    enc.set_dqp(0, None, 0, use_dqp=0)
    enc.set_tiles((6,), (2, 2))
    with pytest.raises(RuntimeError, match="not with tiles in force"):
        enc.set_slices(first)
    enc.set_tiles()
    enc.set_slices(first)
    _assert_slice(_search(hm, enc, cfg, slices[0], finals), slices[0], f"{name} on the context of the refused calls")
    enc.close()
    wpp = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], 1, max_batch=1)
    with pytest.raises(RuntimeError, match="must end with that row"):
        wpp.set_slices([0, 9, 18])
    with pytest.raises(RuntimeError, match="WaveFrontSynchro are not built"):
        wpp.set_slices([0, 9, 12, 21])
    wpp.set_slices()                                       # one slice is no slices: allowed
    wpp.close()


def test_run_begin_outstanding_refuses_set_slices(hm):
    name = SLICE_CASES[0]
    cfg, slices, finals, _, _, extra = load_slices_case(name)
    r = slices[0]
    enc = _encoder(hm, cfg)
    enc.upload(0, _frame(cfg, 0))
    enc.run_begin(0, 0, 1, int(r["qp"]))
    with pytest.raises(RuntimeError, match="a launch is in flight"):
        enc.set_slices(extra["slice_first_ctu"])
    enc.run_wait(0)
    enc.close()


def test_slices_off_again_leaves_no_slice_state(hm):
    """a clip of the default configuration on a context that searched with slices before: with one slice it equals its fixture, slice data
    included; with the slices left on it does not"""
    bitd = {}
    cfg, slices, finals = common.load_ldp_case(UNSLICED, bits=bitd)
    ps = [r for r in slices if int(r["slice_type"]) != 2][:2]
    enc = _encoder(hm, cfg)
    enc.set_slices([0, 3, 6])
    assert enc.lib.hm355_num_substreams(enc.h_) == 3
    with pytest.raises(AssertionError):
        _assert_slice(_search(hm, enc, cfg, ps[0], finals), ps[0], "sliced")
    enc.set_slices()
    assert enc.lib.hm355_num_substreams(enc.h_) == 1 and enc.lib.hm355_num_slices(enc.h_) == 1
    for r in ps:
        _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{UNSLICED} POC {int(r['poc'])} after slices")
        assert enc.last_launch_shape()["tickets"] == enc.num_ctus
    r = slices[0]
    _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{UNSLICED} POC 0 after slices")
    saod = {}
    common.load_ldp_case(UNSLICED, sao=saod)
    rate = np.zeros((3, 8), np.float64)
    enc.deblock_run([(2, int(r["qp"]), r["ref_poc"])])
    (en, _), = enc.sao_run([dict(qp=int(r["qp"]), cabac_init_type=int(r["cabac_init_type"]), depth=saod[0]["depth"], disabled_rate=rate,
                                 chroma_weight=float(r["weight_cb"]), **{"lambda": float(r["lambda"])})])
    (subs, nxt, bins), = enc.encode_slices_run([dict(slice_type=2, qp=int(r["qp"]), sao_enabled=(en[0], en[1]))])
    assert subs == bitd[0]["substreams"] and bins == bitd[0]["num_bins"]
    assert enc.slice_bits_info(0) == [(1, nxt, bins)]
    enc.close()
