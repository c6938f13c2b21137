"""GPU suite (-m gpu): the sticky setters in combination -- hm355_set_tiles / hm355_set_slices with hm355_set_fast_decisions and
hm355_set_motion_search on one context, in both orders, and the LCU-level rate control by CTU range with the switches on -- against clips the real
reference encoded with the same options at once (tests/gen_golden_combo.py).  tests/test_combo_host.py holds the same clips against the kernel
source on the host, so what fails here alone is the launch: the 12-search kernel over pictures x chains independent chains, which a P / B launch
with a tile or slice layout takes by itself only when a fast decision or the full search is on, and the waits between the chains (dep2)."""
import os
import subprocess

import numpy as np
import pytest

import common
import synth
from slices_common import load_slices_case
from test_combo_host import COMBO_CASES, COMBO_TABLE, RC_CASE, combo_settings
from test_gpu_lcu_rate_control import _replay
from test_gpu_tiles import _assert_slice, _search, _want_shape

pytestmark = pytest.mark.gpu
TZ_CASE = "combo_slices_me_ldp"             # no fast decision, no full search: the plan may give it teams of wavefronts
DEFAULT_LDB = "ldb_200x136_8b_qp30"         # the reference's default configuration at the size of fast_all_ldb_200x136_8b_qp30


@pytest.fixture(scope="module")
def hm():
    import hm355
    return hm355


def _apply(enc, s, order="layout_first", without=None):
    """the setters of the clip's features on one context, the tile / slice layout before or after the switches; `without`: that one left out"""
    def layout():
        if "tiles" in s["features"] and without != "tiles":
            enc.set_tiles(s["cols"], s["rows"])
        if "slices" in s["features"] and without != "slices":
            enc.set_slices(s["first"])

    def fast():
        if "fast" in s["features"] and without != "fast":
            enc.set_fast_decisions(*s["fast"])

    def me():
        if "me" in s["features"] and without != "me":
            enc.set_motion_search(*s["me"])
    for step in {"layout_first": (layout, fast, me), "layout_last": (me, fast, layout)}[order]:
        step()


def _chains(s):
    return max(len(s["cols"]) * len(s["rows"]), len(s["first"]))


def _no_teams(s):
    return sum(s["fast"]) > 0 or s["me"][0] == 0


@pytest.mark.parametrize("name,order,team", [(n, o, t) for n in COMBO_CASES for o in ("layout_first", "layout_last") for t in (("0", "1") if n == TZ_CASE else (None,))])
def test_hip_combined_search_matches_reference_fixture(hm, monkeypatch, name, order, team):
    """every picture of the six clips through the search with all the clip's setters applied to one context, the layout first or last: every
    field of every CTU and the reconstruction.  A clip with a fast decision or the full search on runs WITHOUT the HM355_TEAM override, so the
    plan itself takes its P / B launches off the team path: the 12-search kernel, fewWaves 1, one ticket per CTU, groups for `chains` chains."""
    if team is None:
        monkeypatch.delenv("HM355_TEAM", raising=False)
    else:
        monkeypatch.setenv("HM355_TEAM", team)
    cfg, slices, finals, _, _, _ = load_slices_case(name)
    s = combo_settings(name)
    assert _no_teams(s) == (name != TZ_CASE)
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=1)
    _apply(enc, s, order)
    assert enc.lib.hm355_num_substreams(enc.h_) == (enc.num_ctus // ((cfg["width"] + 63) // 64) if cfg["wpp"] else _chains(s))
    assert enc.lib.hm355_num_slices(enc.h_) == len(s["first"])
    n_inter = 0
    for r in slices:
        inter = int(r["slice_type"]) != 2
        _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{name} POC {int(r['poc'])} {order} HM355_TEAM={team}")
        shape = enc.last_launch_shape()
        if inter:
            n_inter += 1
            assert shape == _want_shape(enc.num_ctus, _chains(s), True, team == "1"), f"{name} POC {int(r['poc'])}: {shape}"
            if _no_teams(s):
                assert (shape["kernel"], shape["waves"], shape["few_waves"], shape["tickets"]) == ("search12", 12, 1, enc.num_ctus)
    assert n_inter >= 3
    enc.close()


@pytest.mark.parametrize("name", COMBO_CASES)
def test_hip_combined_closed_loop_on_device_matches_reference(hm, monkeypatch, name):
    """search -> hm355_deblock_run -> hm355_sao_run -> hm355_encode_slices_run -> hm355_ref_from_slot -> the next picture in coding order, with
    all the clip's setters: the finished pictures ('F'), the SAO parameters and slice flags ('A'), the bytes of every substream -- one per tile,
    per slice (with hm355_slice_bits_info) or per CTU row --, the next context table and the bin count ('B')"""
    monkeypatch.delenv("HM355_TEAM", raising=False)
    cfg, slices, finals, saod, bitd, _ = load_slices_case(name)
    s = combo_settings(name)
    sliced = "slices" in s["features"]
    rate = np.zeros((3, 8), np.float64)
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=1)
    _apply(enc, s, "layout_last")
    dev_refs = {}
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
        if sliced:
            assert len(subs) == len(want) == len(s["first"])
            for k, b in enumerate(want):
                assert [subs[k]] == [x for x in b["substreams"] if len(x)], f"{name} POC {poc} slice {k}: slice data bytes"
            info = enc.slice_bits_info(0)
            assert info == [(1, b["next_cabac_init_type"], b["num_bins"]) for b in want], f"{name} POC {poc}: per-slice next table / bins {info}"
        else:
            assert len(want) == 1 and len(subs) == len(want[0]["substreams"])
            assert subs == want[0]["substreams"], f"{name} POC {poc}: slice data bytes differ in substreams {[k for k in range(len(subs)) if subs[k] != want[0]['substreams'][k]]}"
        assert (nxt, bins) == (want[-1]["next_cabac_init_type"], sum(b["num_bins"] for b in want)), f"{name} POC {poc}: next context table / bin count"
        out, _, _ = enc.download(0, want_ctus=False)
        for c in range(3):
            assert np.array_equal(out[c], finals[poc]["rec"][c]), f"{name} POC {poc}: finished picture plane {c}"
        dev_refs[poc] = enc.ref_from_slot(0, poc, st != 2, r["num_ref_idx"], r["ref_poc"], r["ref_long_term"])
    for ref in dev_refs.values():
        enc.ref_release(ref)
    enc.close()


@pytest.mark.parametrize("name", COMBO_CASES)
def test_each_feature_is_needed(hm, monkeypatch, name):
    """per feature of the clip, the first inter picture the reference coded differently without that feature alone -- up to it both reference
    runs saw the same inputs -- searched with that feature's setter left out: it must not equal the fixture"""
    monkeypatch.delenv("HM355_TEAM", raising=False)
    cfg, slices, finals, _, _, _ = load_slices_case(name)
    s = combo_settings(name)
    for f in s["features"]:
        k = next(k for k, r in enumerate(slices) if int(r["slice_type"]) != 2 and int(s["diff"][f][k]) > 0)
        enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=1)
        _apply(enc, s, "layout_first", without=f)
        got = _search(hm, enc, cfg, slices[k], finals)
        with pytest.raises(AssertionError):
            _assert_slice(got, slices[k], f"{name} without {f}")
        enc.close()


@pytest.mark.parametrize("mode", ["whole", "ctu", "row"])
def test_lcu_rate_control_with_fast_decisions_and_search_range(hm, monkeypatch, mode):
    """the clip the reference encoded with the LCU-level rate control, ESD / CFM / ECU and TZ at range 24 at once, under WaveFrontSynchro: whole
    slices, one CTU and one CTU row per hm355_run_ctus call.  Per CTU the bits and the QP the rate model is fed, decisions, motion,
    coefficients, m_phQP, m_bEncodeDQP, slice data and finished pictures against the reference (test_gpu_lcu_rate_control._replay)"""
    monkeypatch.delenv("HM355_TEAM", raising=False)
    s = combo_settings(RC_CASE)
    assert s["features"] == ("fast", "me", "rc")
    assert _replay(hm, RC_CASE, mode, setup=lambda enc: _apply(enc, s)) >= 4


@pytest.mark.parametrize("name,mode,args", [
    ("combo_tiles_fast_me_ldb", "ldb", ("tiles=3x1", "fast=101", "me=0,8,4")), ("combo_tiles_fast_me_ldb", "ldb", ("me=0,8,4", "fast=101", "tiles=3x1")),
    (TZ_CASE, "ldp", ("slices=4", "me=1,24,4")), (TZ_CASE, "ldp", ("me=1,24,4", "slices=4"))], ids=lambda v: "+".join(v) if isinstance(v, tuple) else v)
def test_cpp_host_mirror_with_combined_arguments(tmp_path, name, mode, args):
    """hm355_encmain with the trailing arguments of two and three features, in two orders: from the raw YUV through search, loop filters, slice
    data and device-resident references, every substream of every picture byte for byte as the reference wrote it"""
    cfg, slices, _, _, bitd, _ = load_slices_case(name)
    s = combo_settings(name)
    assert sorted(a.split("=")[0] for a in args) == sorted(s["features"])
    assert args[[a.split("=")[0] for a in args].index("me")] == "me=%d,%d,%d" % s["me"]
    if "fast" in s["features"]:
        assert "fast=%d%d%d" % s["fast"] in args and s["uniform"] and "tiles=%dx%d" % (len(s["cols"]), len(s["rows"])) in args
    else:
        assert f"slices={s['slice_arg']}" in args
    yuv, dump = tmp_path / "in.yuv", tmp_path / "dump.bin"
    synth.write_yuv(str(yuv), cfg["width"], cfg["height"], cfg["bit_depth"], cfg["frames"], cfg["seed"])
    exe = os.path.join(common.ROOT, "hm-16.2_amd", "hm355_encmain")
    env = {k: v for k, v in os.environ.items() if k not in ("HM355_TEAM", "HM355_FAST")}
    subprocess.run([exe, str(yuv), str(cfg["width"]), str(cfg["height"]), str(cfg["bit_depth"]), str(cfg["frames"]), str(s["qp"]), "0", str(dump), mode, *args],
                   check=True, env=env)
    bits = common.read_mirror_bits(str(dump) + ".bits", cfg["frames"])
    assert len(slices) == cfg["frames"]
    for i, r in enumerate(slices):
        want = [x for b in bitd[int(r["poc"])] for x in b["substreams"] if len(x) or len(bitd[int(r["poc"])]) == 1]
        assert bits[i] == want, f"{name} POC {int(r['poc'])}: slice data bytes"


def test_setters_after_a_combined_run_leave_no_state(hm, monkeypatch):
    """tiles, two fast decisions and the full search on one context, the clip's first P / B slice searched, then everything set back.
    A context's picture size is fixed when it is created and no clip of the default configuration exists at 776x72, so the check has two halves.
    On the SAME context the slice searched again with the defaults must equal, field by field, the search of a context that never saw a setter
    (and must not equal the combined fixture).  A SECOND context, created at 200x136 while the first is alive, must reproduce the default
    low-delay B clip of that size -- nothing the setters did lives outside their context."""
    monkeypatch.delenv("HM355_TEAM", raising=False)
    name = "combo_tiles_fast_me_ldb"
    cfg, slices, finals, _, _, _ = load_slices_case(name)
    s = combo_settings(name)
    r = next(r for r in slices if int(r["slice_type"]) != 2)
    enc = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=1)
    _apply(enc, s)
    _assert_slice(_search(hm, enc, cfg, r, finals), r, f"{name} POC {int(r['poc'])}")
    assert enc.last_launch_shape()["kernel"] == "search12"
    enc.set_tiles()
    enc.set_fast_decisions(0, 0, 0)
    enc.set_motion_search(1, 64, 4)
    assert enc.lib.hm355_num_substreams(enc.h_) == 1
    got = _search(hm, enc, cfg, r, finals)
    assert (enc.last_launch_shape()["kernel"], enc.last_launch_shape()["tickets"]) == ("team", enc.num_ctus)      # the plan's own choice again
    with pytest.raises(AssertionError):
        _assert_slice(got, r, "defaults")
    fresh = hm.Encoder(cfg["width"], cfg["height"], cfg["bit_depth"], cfg["wpp"], max_batch=1)
    want = _search(hm, fresh, cfg, r, finals)
    fresh.close()
    for k in (1, 2):
        for f in want[k].dtype.names:
            assert np.array_equal(got[k][f], want[k][f]), f"after the setters were set back: {f} differs from a context that never saw one"
    for c in range(3):
        assert np.array_equal(got[0][c], want[0][c]), f"after the setters were set back: reconstruction plane {c}"
    dcfg, dslices, dfinals = common.load_ldp_case(DEFAULT_LDB)
    other = hm.Encoder(dcfg["width"], dcfg["height"], dcfg["bit_depth"], dcfg["wpp"], max_batch=1)
    for d in dslices:
        _assert_slice(_search(hm, other, dcfg, d, dfinals), d, f"{DEFAULT_LDB} POC {int(d['poc'])} next to a context that ran {name}")
    other.close()
    enc.close()
