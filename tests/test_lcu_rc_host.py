"""CPU suite: the host side of the LCU-level rate control (stage 2) -- the kernel source's per-CTU lambda path on the host twin,
and the C ABI record of the rate-control feedback against its ctypes mirror."""
import os
import subprocess

import numpy as np

import common

ROOT = common.ROOT


def test_hostsim_lcu_rate_control_matches_reference(tmp_path):
    """The kernel source (hm355_core.h) for the host, armed with DqpPic and a CtuRc record per CTU built from the 'L' record of the all-intra
    10-bit clip, reproduces the reference's first picture: decisions, coefficients, costs, reconstruction, m_phQP -- and the feedback record
    process_ctu leaves for updateAfterCTU.  Debugging aid: the GPU tests are the gate."""
    import gen_golden
    import synth
    cfg, slices, _ = common.load_ldp_case("rc2_i_256x192_10b")
    r = slices[0]
    w, h, bd = cfg["width"], cfg["height"], cfg["bit_depth"]
    planes = synth.frame(w, h, bd, int(r["poc"]), cfg["seed"])
    (tmp_path / "in.yuv").write_bytes(b"".join(np.ascontiguousarray(p, "<u2").tobytes() for p in planes))
    (tmp_path / "qp.i8").write_bytes(np.asarray(r["lcu_rc"]["ctu_qp"]).astype(np.int8).tobytes())
    (tmp_path / "lambda.f64").write_bytes(np.asarray(r["lcu_rc"]["ctu_lambda"], "<f8").tobytes())
    exe = common.build_hostsim(tmp_path, "hostsim_rc")
    dump = tmp_path / "dump.bin"
    subprocess.run([str(exe), str(tmp_path / "in.yuv"), str(w), str(h), str(bd), str(int(r["qp"])), repr(float(r["lambda"])), repr(float(r["weight_cb"])),
                    str(cfg["wpp"]), str(int(r["dqp"]["dqp_flag_in"])), str(tmp_path / "qp.i8"), str(tmp_path / "lambda.f64"), str(dump)], check=True)
    (ctus, rec), = gen_golden.parse_dump(str(dump))
    common.assert_ctus_equal(ctus, common.split_fixture_ctus(r["ctus"])[0], "hostsim_rc")
    common.assert_rec_equal(common.split_rec(rec, w, h), np.concatenate([r["rec"][c].reshape(-1) for c in range(3)]), w, h, "hostsim_rc")
    rc = np.frombuffer((tmp_path / "dump.bin.rc").read_bytes(), np.dtype([("bits", "<i4"), ("qp", "<i4"), ("phqp", "i1", 256)]))
    m = common.inside_mask(len(ctus), w, h)
    assert np.array_equal(rc["phqp"][m], r["dqp"]["qp"][m]), "hostsim_rc: m_phQP"
    assert np.array_equal(rc["bits"], r["ctus"]["total_bits"].astype(np.int32)), "hostsim_rc: feedback bits"
    assert np.array_equal(rc["qp"], r["dqp"]["qp"][:, 0].astype(np.int32)), "hostsim_rc: feedback QP (an I slice codes every CTU)"
    assert not np.any(np.isclose(r["lcu_rc"]["ctu_lambda"], float(r["lambda"]))), "the CTUs should be searched with lambdas other than the slice's"


def test_ctu_rc_record_layout_matches_ctypes(tmp_path):
    """hm355_ctu_rc as a C compiler lays it out from include/hm355.h equals the ctypes mirror in hm355.py"""
    import hm355
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hm355.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(hm355_ctu_rc), offsetof(hm355_ctu_rc, bits), offsetof(hm355_ctu_rc, qp)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    size, off_bits, off_qp = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == __import__("ctypes").sizeof(hm355.CtuRc) == hm355.CTU_RC_DTYPE.itemsize
    assert (off_bits, off_qp) == (hm355.CtuRc.bits.offset, hm355.CtuRc.qp.offset)
    assert (off_bits, off_qp) == (hm355.CTU_RC_DTYPE.fields["bits"][1], hm355.CTU_RC_DTYPE.fields["qp"][1])


def _at(addr, dtype, count):
    """what a pointer field of a descriptor points to (None for a null pointer)"""
    import ctypes
    return np.frombuffer(ctypes.string_at(addr, count * np.dtype(dtype).itemsize), dtype).copy() if addr else None


def _desc_image(s, w, h):
    """an hm355_inter_slice_desc as nested plain values, every pointer replaced by the contents it points to"""
    n = ((w + 63) // 64) * ((h + 63) // 64) * 256
    img = {k: getattr(s, k) for k in ("poc", "cabac_init_type", "col_from_l0", "col_ref_idx", "tmvp", "mvd_l1_zero", "max_merge_cand", "check_ldc",
                                      "lambda_motion_sad", "lambda_motion_sse")}
    img.update(slice_type=s.base.slice_type, qp=s.base.qp, lambda_=s.base.lambda_, chroma_weight=s.base.chroma_weight, num_ref_idx=tuple(s.num_ref_idx))
    for l in range(2):
        for i in range(16):
            img["dev_ref", l, i] = s.dev_ref[l][i]
            if not s.ref[l][i]:
                img["ref", l, i] = None
                continue
            r = s.ref[l][i].contents
            img["ref", l, i] = dict(poc=r.poc, slice_type=r.slice_type, long_term=r.long_term, num_ref=tuple(r.num_ref),
                                    ref_poc=np.array(r.ref_poc), ref_lt=np.array(r.ref_lt), pred_mode=_at(r.pred_mode, np.uint8, n),
                                    plane=[_at(r.plane[c], np.uint16, (w >> (c > 0)) * (h >> (c > 0))) for c in range(3)],
                                    mv=[_at(r.mv[k], np.int16, 2 * n) for k in range(2)], ref_idx=[_at(r.ref_idx[k], np.int8, n) for k in range(2)])
    return img


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


class _RecordingLib:
    """stands in for libhm355.so: keeps an image of every inter slice descriptor the binding hands to the library"""
    def __init__(self, w, h):
        self.size, self.begun, self.batch = (w, h), [], []

    def hm355_create(self, cfg, out):
        return 0

    def hm355_slice_begin_inter(self, ctx, slot, desc):
        self.begun.append(_desc_image(desc._obj, *self.size))
        return 0

    def hm355_compress_slices_inter(self, ctx, n, descs, *outputs):
        self.batch.append(([_desc_image(descs[k], *self.size) for k in range(n)],
                           [[__import__("ctypes").addressof(descs[k].ref[l][i].contents) if descs[k].ref[l][i] else 0 for l in range(2) for i in range(16)] for k in range(n)]))
        return 0


def test_inter_slice_descriptor_is_built_once_for_both_entry_points():
    """No GPU, no library: hm355_inter_slice_desc / hm355_ref_pic of a recorded B slice as Encoder.slice_begin_inter and Encoder.compress_inter_batch
    hand them to the library are the same record, and that record holds the fixture's values field by field -- every motion field and reference
    list of a host reference picture included, pointers followed to what they point to.  Two jobs that share a ref_pics dict point at the same
    hm355_ref_pic records (the library uploads them once); a device-resident reference goes into dev_ref and leaves ref null."""
    import hm355
    cfg, slices, finals = common.load_ldp_case("ra_192x128_10b_qp32")
    w, h = cfg["width"], cfg["height"]
    r = next(s for s in slices if int(s["slice_type"]) == 0 and s["num_ref_idx"][1] > 0)
    sp, refs = common.ldp_slice_inputs(r, finals)
    planes = [np.zeros((h >> (c > 0), w >> (c > 0)), np.uint16) for c in range(3)]
    lib = _RecordingLib(w, h)
    enc = hm355.Encoder(w, h, cfg["bit_depth"], cfg["wpp"], 2, lib=lib)
    enc.slice_begin_inter(0, sp, refs)
    enc.compress_inter_batch([(planes, sp, refs), (planes, sp, refs), (planes, sp, dict(refs))])
    enc.h_ = None
    (begun,), ((batch, addrs),) = lib.begun, lib.batch
    direct, _ = hm355._inter_slice_desc(sp, refs)
    for got in batch + [_desc_image(direct, w, h)]:
        assert _same(got, begun)
    assert addrs[0] == addrs[1] and any(addrs[0]), "jobs that share a ref_pics dict share its hm355_ref_pic records"
    assert all(a != b for a, b in zip(addrs[0], addrs[2]) if a), "another dict object is another set of records"
    for k in ("poc", "cabac_init_type", "col_from_l0", "col_ref_idx", "tmvp", "mvd_l1_zero", "max_merge_cand", "check_ldc", "lambda_motion_sad", "lambda_motion_sse",
              "slice_type", "qp"):
        assert begun[k] == int(r[k]), k
    assert (begun["lambda_"], begun["chroma_weight"], begun["num_ref_idx"]) == (float(r["lambda"]), float(r["weight_cb"]), tuple(r["num_ref_idx"]))
    for l in range(2):
        for i in range(16):
            got = begun["ref", l, i]
            assert begun["dev_ref", l, i] is None
            if i >= r["num_ref_idx"][l]:
                assert got is None
                continue
            f = finals[int(r["ref_poc"][l][i])]; m = f["motion"]
            assert (got["poc"], got["slice_type"], got["long_term"], got["num_ref"]) == (f["poc"], f["slice_type"], 0, tuple(f["num_ref_idx"]))
            assert np.array_equal(got["ref_poc"], f["ref_poc"]) and np.array_equal(got["ref_lt"], f["ref_long_term"])
            assert np.array_equal(got["pred_mode"], m["pred_mode"].reshape(-1))
            for c in range(3):
                assert np.array_equal(got["plane"][c], f["rec"][c].reshape(-1))
            for k in range(2):
                assert np.array_equal(got["mv"][k], m[f"mv{k}"].reshape(-1)) and np.array_equal(got["ref_idx"][k], m[f"ref_idx{k}"].reshape(-1))
    dev = {p: {"dev": 0x1000 + 16 * k} for k, p in enumerate(refs)}
    img = _desc_image(hm355._inter_slice_desc(sp, dev)[0], w, h)
    for l in range(2):
        for i in range(16):
            want = dev[int(r["ref_poc"][l][i])]["dev"] if i < r["num_ref_idx"][l] else None
            assert img["ref", l, i] is None and img["dev_ref", l, i] == want


def test_inter_slice_params_gives_the_dicts_its_callers_spelled_out():
    """hm355.inter_slice_params for the arguments of its six call sites equals the dict each of them held as a literal before the helper existed
    (copied here): keys, integers and float lambdas exactly.  The three sites that build an 'S' record hand the record to ldp_slice_inputs, so
    their literal is compared after that adapter, as the encoder saw it."""
    import math
    import hm355 as hm
    z = np.zeros((2, 16), np.int32)

    def same(got, want):
        assert got.keys() == want.keys()
        for k, v in want.items():
            assert (got[k] is v) if isinstance(v, np.ndarray) else (type(got[k]) is type(v) and got[k] == v), k

    for kind in "PB":                                                           # tests/test_gpu_parity.py, fresh inputs
        qp = 30
        lam = 0.4624 * 2.0 ** ((qp + 2 - 12) / 3.0) * 2.0
        srec = {"poc": 2, "slice_type": 1 if kind == "P" else 0, "qp": qp + 2, "lambda": lam, "weight_cb": hm.intra_lambda(qp + 2)[1],
                "cabac_init_type": 1 if kind == "P" else 0, "num_ref_idx": (2, 0 if kind == "P" else 2), "ref_poc": z, "col_from_l0": 0 if kind == "B" else 1,
                "col_ref_idx": 0, "tmvp": 1, "mvd_l1_zero": 0, "max_merge_cand": 5, "check_ldc": 0 if kind == "B" else 1,
                "lambda_motion_sad": int(math.floor(65536.0 * math.sqrt(lam))), "lambda_motion_sse": int(math.floor(65536.0 * lam))}
        same(hm.inter_slice_params(kind, qp + 2, lam, 2, (2, 0 if kind == "P" else 2), z, col_from_l0=0 if kind == "B" else 1, check_ldc=0 if kind == "B" else 1),
             common.ldp_slice_inputs(srec, None, {})[0])
    for kind, pocs in (("P", [3, 2, 1, 0]), ("B", [0, 8])):                     # tests/test_gpu_parity.py, full size
        qps, cur_poc = 32 + (3 if kind == "P" else 2), 4
        lam = (0.4624 if kind == "P" else 0.3536) * 2.0 ** ((qps - 12) / 3.0) * min(4.0, max(2.0, (qps - 12) / 6.0))
        srec = {"poc": cur_poc, "slice_type": 1 if kind == "P" else 0, "qp": qps, "lambda": lam, "weight_cb": hm.intra_lambda(qps)[1],
                "cabac_init_type": 1 if kind == "P" else 0, "num_ref_idx": (len(pocs), 0 if kind == "P" else len(pocs)), "ref_poc": z, "col_from_l0": 1,
                "col_ref_idx": 0, "tmvp": 1, "mvd_l1_zero": 0, "max_merge_cand": 5, "check_ldc": 1 if kind == "P" else 0,
                "lambda_motion_sad": int(math.floor(65536.0 * math.sqrt(lam))), "lambda_motion_sse": int(math.floor(65536.0 * lam))}
        same(hm.inter_slice_params(kind, qps, lam, cur_poc, (len(pocs), 0 if kind == "P" else len(pocs)), z, check_ldc=1 if kind == "P" else 0),
             common.ldp_slice_inputs(srec, None, {})[0])
    qp = 46                                                                     # tests/test_gpu_lcu_rate_control.py
    lam = 0.4624 * 2.0 ** ((qp - 12) / 3.0)
    same(hm.inter_slice_params("P", qp, lam, 1, (1, 0), z),
         dict(slice_type=1, qp=qp, chroma_weight=hm.intra_lambda(qp)[1], poc=1, cabac_init_type=1, num_ref_idx=(1, 0), ref_poc=z,
              col_from_l0=1, col_ref_idx=0, tmvp=1, mvd_l1_zero=0, max_merge_cand=5, check_ldc=1,
              lambda_motion_sad=int(np.floor(65536.0 * np.sqrt(lam))), lambda_motion_sse=int(np.floor(65536.0 * lam)), **{"lambda": lam}))
    for kind, qp, l0, l1, cit, cfl0, tmvp, mvd0, mrg, ldc in (("P", 23, [2, 6], [6], 0, 1, 0, 0, 3, 0), ("B", 37, [2, 0], [2], 1, 0, 1, 1, 1, 1)):   # tools/fuzz_parity.py
        cur_poc = 4
        lam = 0.4624 * 2.0 ** ((qp - 12) / 3.0) * 2.0
        srec = {"poc": cur_poc, "slice_type": 1 if kind == "P" else 0, "qp": qp, "lambda": lam, "weight_cb": hm.intra_lambda(qp)[1],
                "cabac_init_type": cit, "num_ref_idx": (len(l0), len(l1) if kind == "B" else 0), "ref_poc": z,
                "col_from_l0": cfl0, "col_ref_idx": 0, "tmvp": tmvp, "mvd_l1_zero": mvd0,
                "max_merge_cand": mrg, "check_ldc": ldc,
                "lambda_motion_sad": int(math.floor(65536.0 * math.sqrt(lam))), "lambda_motion_sse": int(math.floor(65536.0 * lam))}
        same(hm.inter_slice_params(kind, qp, lam, cur_poc, (len(l0), len(l1) if kind == "B" else 0), z,
                                   cabac_init_type=cit, col_from_l0=cfl0, tmvp=tmvp, mvd_l1_zero=mvd0, max_merge_cand=mrg, check_ldc=ldc),
             common.ldp_slice_inputs(srec, None, {})[0])
    qp, nref = 32, 4                                                            # tools/inter_batch_timing.py (and inter_timing.py)
    lam = 0.4624 * 2.0 ** ((qp + 3 - 12) / 3.0) * min(4.0, max(2.0, (qp + 3 - 12) / 6.0))
    sp = dict(qp=qp + 3, chroma_weight=hm.intra_lambda(qp + 3)[1], poc=nref, cabac_init_type=1, num_ref_idx=(nref, 0), ref_poc=z,
              col_from_l0=1, col_ref_idx=0, tmvp=1, mvd_l1_zero=0, max_merge_cand=5, check_ldc=1,
              lambda_motion_sad=int(math.floor(65536.0 * math.sqrt(lam))), lambda_motion_sse=int(math.floor(65536.0 * lam)))
    sp["lambda"] = lam
    got = hm.inter_slice_params("P", qp + 3, lam, nref, (nref, 0), z)
    assert got.pop("slice_type") == 1              # this one site left the slice type to the binding's default, sp.get("slice_type", 1): the helper states it
    same(got, sp)
    dev = {0: {"dev": 1}}
    assert bytes(hm._inter_slice_desc(sp, dev)[0]) == bytes(hm._inter_slice_desc(dict(got, slice_type=1), dev)[0])
    qp = 32                                                                     # tools/lcu_rc_timing.py
    lam = 0.4624 * 2.0 ** ((qp - 12) / 3.0)
    same(hm.inter_slice_params("P", qp, lam, 1, (1, 0), z),
         dict(slice_type=1, qp=qp, chroma_weight=hm.intra_lambda(qp)[1], poc=1, cabac_init_type=1, num_ref_idx=(1, 0), ref_poc=z,
              col_from_l0=1, col_ref_idx=0, tmvp=1, mvd_l1_zero=0, max_merge_cand=5, check_ldc=1,
              lambda_motion_sad=int(math.floor(65536.0 * math.sqrt(lam))), lambda_motion_sse=int(math.floor(65536.0 * lam)), **{"lambda": lam}))
