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
    exe = tmp_path / "hostsim_rc"
    subprocess.run(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-w", "-o", str(exe), os.path.join(ROOT, "tests", "hostsim", "hostsim_rc.cpp")], check=True)
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
