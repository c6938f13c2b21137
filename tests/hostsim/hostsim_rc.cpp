// DEBUGGING AID, NOT PRODUCT: the LCU-level rate control path of hm-16.2_amd/csrc/hm355_core.h (DqpPic with a CtuRc record per CTU,
// process_ctu's per-CTU lambda and its feedback record) compiled for the host with one "lane" (see hostsim.cpp), for one I picture.
// The records are built by hm355_ctu_rc_record (hm355_host_common.h) exactly as the library builds them.  The team code is not run.
//   hostsim_rc <in.yuv> <w> <h> <bitdepth> <qp> <lambda> <chroma_weight> <wpp> <dqp_flag_in> <ctu_qp.i8> <ctu_lambda.f64> <dump.bin>
// dump.bin: the HMD1 dump of hostsim.cpp (one picture); dump.bin.rc: per CTU int32 bits, int32 QP (CtuRcOut), then int8 m_phQP[256]
#define HM355_HOSTSIM 1
#include "../../hm-16.2_amd/csrc/hm355_core.h"
#include "../../hm-16.2_amd/csrc/hm355_host_common.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

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
  Params P; memset(&P, 0, sizeof(P));
  P.width = w; P.height = h; P.bitDepth = bd; P.wpp = wpp; P.wCtu = (w + 63) / 64; P.hCtu = (h + 63) / 64;
  P.stride[0] = P.wCtu * 64; P.stride[1] = P.stride[2] = P.wCtu * 32;
  const int nctu = P.wCtu * P.hCtu;
  Tables *tab = new Tables; hm355_build_tables(tab); P.tab = tab;
  P.ws = (WorkSpace *)calloc(1, sizeof(WorkSpace));
  FrameBuf fb; memset(&fb, 0, sizeof(fb));
  FILE *fi = fopen(argv[1], "rb");
  if (!fi) { perror("open"); return 1; }
  for (int c = 0; c < 3; c++) {
    const size_t n = (size_t)P.stride[c] * P.hCtu * (c ? 32 : 64);
    fb.org[c] = (Pel *)calloc(n, sizeof(Pel)); fb.rec[c] = (Pel *)calloc(n, sizeof(Pel));
    const int pw = w >> (c ? 1 : 0), ph = h >> (c ? 1 : 0);
    for (int y = 0; y < ph; y++) for (int x = 0; x < pw; x++) {
      unsigned v;
      if (bd == 8) { unsigned char t; if (fread(&t, 1, 1, fi) != 1) return 3; v = t; } else { unsigned short t; if (fread(&t, 2, 1, fi) != 1) return 3; v = t; }
      fb.org[c][y * P.stride[c] + x] = (Pel)v;
    }
  }
  fclose(fi);
  fb.meta = (CtuMeta *)calloc(nctu, sizeof(CtuMeta)); fb.coef = (TCoeff *)calloc((size_t)nctu * HM_COEF_CTU, sizeof(TCoeff));
  fb.stat = (CtuStat *)calloc(nctu, sizeof(CtuStat)); fb.endState = (Cabac *)calloc(nctu, sizeof(Cabac));
  hm355_fill_slice_params(&fb, bd, qp, lambda, cw);
  // cu_qp_delta state as the library's dqp_prepare builds it, with the rate control's record of every CTU
  std::vector<int8_t> ctuQp(nctu); std::vector<double> ctuLambda(nctu);
  if (!read_all(argv[10], ctuQp.data(), nctu) || !read_all(argv[11], ctuLambda.data(), sizeof(double) * nctu)) { fprintf(stderr, "bad rate control inputs\n"); return 4; }
  std::vector<CtuDqp> out(nctu); std::vector<uint8_t> rowFlag(P.hCtu, 0); std::vector<CtuRc> rc(nctu); std::vector<CtuRcOut> rcOut(nctu);
  for (int a = 0; a < nctu; a++) rc[a] = hm355_ctu_rc_record(bd, ctuQp[a], ctuLambda[a], cw);
  DqpPic *dp = new DqpPic; memset(dp, 0, sizeof(*dp));
  dp->flagIn = flagIn; dp->sliceQp = qp; dp->ctuQp = ctuQp.data(); dp->out = out.data(); dp->rowFlag = rowFlag.data();
  for (int q = -12; q <= 51; q++) {
    FrameBuf t; memset(&t, 0, sizeof(t));
    hm355_fill_slice_params(&t, bd, q, lambda, cw);
    QpTab &e = dp->tab[q + 12];
    for (int k = 0; k < 2; k++) { e.qpPer[k] = t.qpPer[k]; e.qpRem[k] = t.qpRem[k]; e.rdFactor[k] = t.rdFactor[k]; for (int l = 0; l < 4; l++) e.errScale[k][l] = t.errScale[k][l]; }
  }
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
  fwrite("HMD1", 1, 4, fo);
  uint32_t hdr[5] = { (uint32_t)w, (uint32_t)h, (uint32_t)bd, 64, 1u }; fwrite(hdr, 4, 5, fo);
  uint32_t u[2] = { 0u, (uint32_t)nctu }; fwrite(u, 4, 2, fo);
  for (int a = 0; a < nctu; a++) {
    fwrite(&fb.stat[a].cost, 8, 1, fo); fwrite(&fb.stat[a].bits, 4, 1, fo); fwrite(&fb.stat[a].dist, 4, 1, fo);
    fwrite(&fb.meta[a], 1, sizeof(CtuMeta), fo);
    fwrite(fb.coef + (size_t)a * HM_COEF_CTU, 4, HM_COEF_CTU, fo);
  }
  for (int c = 0; c < 3; c++) {
    const int pw = w >> (c ? 1 : 0), ph = h >> (c ? 1 : 0);
    for (int y = 0; y < ph; y++) for (int x = 0; x < pw; x++) { unsigned short v = (unsigned short)fb.rec[c][y * P.stride[c] + x]; fwrite(&v, 2, 1, fo); }
  }
  for (int a = 0; a < nctu; a++) {
    fwrite(&rcOut[a], sizeof(CtuRcOut), 1, fr);
    int8_t q[256];
    for (int z = 0; z < 256; z++) q[z] = z < out[a].firstZ ? out[a].refQp : out[a].qp;
    fwrite(q, 1, 256, fr);
  }
  fclose(fo); fclose(fr);
  return 0;
}
