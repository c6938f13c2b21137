// DEBUGGING AID, NOT PRODUCT: the LCU-level rate control path of hm-16.2_amd/csrc/hm355_core.h (DqpPic with a CtuRc record per CTU,
// process_ctu's per-CTU lambda and its feedback record) compiled for the host with one "lane" (see hostsim.cpp), for one I picture.
// The records are built by hm355_ctu_rc_record (hm355_host_common.h) exactly as the library builds them.  The team code is not run.
//   hostsim_rc <in.yuv> <w> <h> <bitdepth> <qp> <lambda> <chroma_weight> <wpp> <dqp_flag_in> <ctu_qp.i8> <ctu_lambda.f64> <dump.bin>
// dump.bin: the HMD1 dump of hostsim.cpp (one picture); dump.bin.rc: per CTU int32 bits, int32 QP (CtuRcOut), then int8 m_phQP[256]
#include "hostsim_common.h"
#include <string>

static bool read_all(const char *path, void *dst, size_t bytes)
{
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  const bool ok = fread(dst, 1, bytes, f) == bytes;
  fclose(f);
  return ok;
}

int main(int argc, char **argv)
{
  if (argc < 13) { fprintf(stderr, "usage: %s in.yuv w h bd qp lambda chroma_weight wpp dqp_flag_in ctu_qp.i8 ctu_lambda.f64 dump.bin\n", argv[0]); return 2; }
  const int w = atoi(argv[2]), h = atoi(argv[3]), bd = atoi(argv[4]), qp = atoi(argv[5]), wpp = atoi(argv[8]), flagIn = atoi(argv[9]);
  const double lambda = atof(argv[6]), cw = atof(argv[7]);
  Params P; hostsim_params(P, w, h, bd, wpp);
  const int nctu = P.wCtu * P.hCtu;
  FrameBuf fb; hostsim_alloc_frame(fb, P);
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) { perror("open"); return 1; }
  if (!hostsim_read_yuv(fi, fb, P)) return 3;
  fclose(fi);
  hm355_fill_slice_params(&fb, bd, qp, lambda, cw);
  // cu_qp_delta state as the library's dqp_prepare builds it (hm355_fill_qp_tab), with the rate control's record of every CTU
  std::vector<int8_t> ctuQp(nctu); std::vector<double> ctuLambda(nctu);
  if (!read_all(argv[10], ctuQp.data(), nctu) || !read_all(argv[11], ctuLambda.data(), sizeof(double) * nctu)) { fprintf(stderr, "bad rate control inputs\n"); return 4; }
  std::vector<CtuDqp> out(nctu); std::vector<uint8_t> rowFlag(P.hCtu, 0); std::vector<CtuRc> rc(nctu); std::vector<CtuRcOut> rcOut(nctu);
  for (int a = 0; a < nctu; a++) rc[a] = hm355_ctu_rc_record(bd, ctuQp[a], ctuLambda[a], cw);
  DqpPic *dp = new DqpPic; memset(dp, 0, sizeof(*dp));
  dp->flagIn = flagIn; dp->sliceQp = qp; dp->ctuQp = ctuQp.data(); dp->out = out.data(); dp->rowFlag = rowFlag.data();
  hm355_fill_qp_tab(dp->tab, bd, lambda, cw);
  dp->rc = rc.data(); dp->rcOut = rcOut.data(); dp->firstCtu = 0;
  fb.dqp = dp;
  P.frames = &fb;
  // coding order, one CTU at a time: a row start under WaveFrontSynchro always finds its predecessor finished, so the real m_bEncodeDQP is used
  static Shared sh;
  for (int a = 0; a < nctu; a++) {
    dp->firstCtu = a;
    WorkItem it = {0, a % P.wCtu, a / P.wCtu, 0};
    process_ctu(&sh, &P, &it, 0);
  }
  FILE *fo = fopen(argv[12], "wb"), *fr = fopen((std::string(argv[12]) + ".rc").c_str(), "wb");
  if (!fo || !fr) { perror("open"); return 1; }
  hostsim_write_hmd1_header(fo, P, 1);
  hostsim_write_hmd1_picture(fo, P, fb, 0);
  for (int a = 0; a < nctu; a++) {
    fwrite(&rcOut[a], sizeof(CtuRcOut), 1, fr);
    int8_t q[256];
    for (int z = 0; z < 256; z++) q[z] = z < out[a].firstZ ? out[a].refQp : out[a].qp;
    fwrite(q, 1, 256, fr);
  }
  fclose(fo); fclose(fr);
  return 0;
}
