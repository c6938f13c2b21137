// DEBUGGING AID, NOT PRODUCT: hostsim_me.cpp's self-checking replay of an HMD2 record stream (every slice re-run with the slice parameters and
// reference pictures of its record and compared in place) with the slice partition of hm355_set_slices taken from the command line and put into
// Params::slice as the library puts it -- I pictures too, CTUs in the order of hm355_build_schedule.  Search only: 'A' and 'B' records are skipped.
// The stream holds one 'S' record per picture: the complete picture, as the reference leaves it after the last slice.
//   hostsim_slices <in.yuv> <dump2.bin> <w> <h> <bitdepth> <first CTUs, e.g. 0,8,16>       ("0": one slice, Params::slice NULL)
//                  [fast=<esd><cfm><ecu>] [me=<fast>,<range>,<bipred>] [max_inter_slices=<n>]   (hostsim_common.h: hostsim_switch_arg; n counts pictures here)
// exit code 0 = every picture replayed is bit-exact
#include "hostsim_common.h"
#include <map>

struct FinalPic { int poc, sliceType; std::vector<Pel> buf[3]; int stride[3]; int numRef[2]; int refPoc[2][16], refLT[2][16]; std::vector<uint8_t> pm; std::vector<MvD> mv[2]; std::vector<int8_t> ri[2]; };
static const unsigned char *g_p; static size_t g_n, g_off;
template <class T> static T rd() { T v; memcpy(&v, g_p + g_off, sizeof(T)); g_off += sizeof(T); return v; }
static void rdbuf(void *d, size_t n) { memcpy(d, g_p + g_off, n); g_off += n; }
static std::vector<int> int_list(const char *s) { std::vector<int> v; for (const char *p = s; *p;) { v.push_back(atoi(p)); while (*p && *p != ',') p++; if (*p) p++; } return v; }

int main(int argc, char **argv)
{
  if (argc < 7) { fprintf(stderr, "usage: %s in.yuv dump2.bin w h bd first_ctus\n", argv[0]); return 2; }
  const int w = atoi(argv[3]), h = atoi(argv[4]), bd = atoi(argv[5]);
  FILE *fy = fopen(argv[1], "rb"), *fd = fopen(argv[2], "rb");
  if (!fy || !fd) { perror("open"); return 1; }
  fseek(fd, 0, SEEK_END); g_n = ftell(fd); fseek(fd, 0, SEEK_SET);
  std::vector<unsigned char> data(g_n); if (fread(data.data(), 1, g_n, fd) != g_n) return 1;
  g_p = data.data(); g_off = 4;
  Params P; hostsim_params(P, w, h, bd, 0);
  hm355_slice_tables slices;
  const std::vector<int> first = int_list(argv[6]);
  { const char *why = hm355_build_slices(P.wCtu, P.hCtu, 0, (int)first.size(), first.data(), &slices);
    if (why) { fprintf(stderr, "slices: %s\n", why); return 2; }
    if (slices.count() > 1) { P.slice = slices.ctu.data(); P.sliceStart = slices.start.data(); P.numSlices = slices.count(); } }
  int maxInter = 1 << 30, nInter = 0;
  for (int i = 7; i < argc; i++) if (!hostsim_switch_arg(argv[i], P, maxInter)) { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
  const int nctu = P.wCtu * P.hCtu;
  std::map<int, FinalPic> finals;
  const size_t frameBytes = (size_t)w * h * 3 / 2 * (bd == 8 ? 1 : 2);
  int bad = 0, nS = 0;
  static Shared sh;
  while (g_off < g_n) {
    const char tag = (char)rd<unsigned char>();
    if (tag == 'F') {
      FinalPic f; f.poc = rd<int32_t>();
      for (int c = 0; c < 3; c++) {
        const int cw = w >> (c ? 1 : 0), ch = h >> (c ? 1 : 0), mg = HM_REF_MARGIN >> (c ? 1 : 0), st = cw + 2 * mg;
        f.stride[c] = st; f.buf[c].resize((size_t)st * (ch + 2 * mg));
        std::vector<uint16_t> pl((size_t)cw * ch); rdbuf(pl.data(), pl.size() * 2);
        for (int y = -mg; y < ch + mg; y++) for (int x = -mg; x < cw + mg; x++) {   // TComPicYuv::extendPicBorder
          const int sy = y < 0 ? 0 : (y >= ch ? ch - 1 : y), sx = x < 0 ? 0 : (x >= cw ? cw - 1 : x);
          f.buf[c][(size_t)(y + mg) * st + x + mg] = (Pel)pl[(size_t)sy * cw + sx];
        }
      }
      f.sliceType = rd<int32_t>(); f.numRef[0] = rd<int32_t>(); f.numRef[1] = rd<int32_t>();
      rdbuf(f.refPoc, sizeof(f.refPoc)); rdbuf(f.refLT, sizeof(f.refLT));
      const uint32_t n = rd<uint32_t>();
      f.pm.resize((size_t)n * 256); for (int l = 0; l < 2; l++) { f.mv[l].resize((size_t)n * 256); f.ri[l].resize((size_t)n * 256); }
      for (uint32_t a = 0; a < n; a++) {
        rdbuf(&f.pm[(size_t)a * 256], 256);
        for (int l = 0; l < 2; l++) { rdbuf(&f.mv[l][(size_t)a * 256], 1024); rdbuf(&f.ri[l][(size_t)a * 256], 256); }
      }
      finals[f.poc] = f;
      continue;
    }
    if (tag == 'A') { g_off += 16; const uint32_t n = rd<uint32_t>(); g_off += (size_t)n * 105 * 4; continue; }
    if (tag == 'B') { g_off += 4; const uint32_t ns = rd<uint32_t>(); for (uint32_t k = 0; k < ns; k++) { const uint32_t nb = rd<uint32_t>(); g_off += nb; } g_off += 8; continue; }
    if (tag != 'S') { fprintf(stderr, "bad tag at %zu\n", g_off - 1); return 1; }
    const int poc = rd<int32_t>(), sliceType = rd<int32_t>(), qp = rd<int32_t>(); rd<int32_t>(); rd<int32_t>();
    const double lambda = rd<double>(); rd<double>(); const double wcb = rd<double>(); rd<double>();
    const uint32_t lmSAD = rd<uint32_t>(), lmSSE = rd<uint32_t>();
    int numRef[2]; numRef[0] = rd<int32_t>(); numRef[1] = rd<int32_t>();
    int refPoc[2][16], refLT[2][16]; rdbuf(refPoc, sizeof(refPoc)); rdbuf(refLT, sizeof(refLT));
    int misc[7]; rdbuf(misc, sizeof(misc)); g_off += 64;
    const uint32_t n = rd<uint32_t>();
    std::vector<CtuStat> wantStat(n); std::vector<CtuMeta> wantMeta(n); std::vector<InterMeta> wantIm(n); std::vector<TCoeff> wantCoef((size_t)n * HM_COEF_CTU);
    for (uint32_t a = 0; a < n; a++) {
      wantStat[a].cost = rd<double>(); wantStat[a].bits = rd<uint32_t>(); wantStat[a].dist = rd<uint32_t>();
      rdbuf(&wantMeta[a], 12 * 256);
      InterMeta &im = wantIm[a];
      rdbuf(im.skip, 256); rdbuf(im.mrg, 256); rdbuf(im.mrgIdx, 256); rdbuf(im.interDir, 256);
      for (int l = 0; l < 2; l++) { rdbuf(im.mv[l], 1024); rdbuf(im.mvd[l], 1024); rdbuf(im.refIdx[l], 256); rdbuf(im.mvpIdx[l], 256); rdbuf(im.mvpNum[l], 256); }
      rdbuf(&wantCoef[(size_t)a * HM_COEF_CTU], HM_COEF_CTU * 4);
    }
    std::vector<uint16_t> wantRec[3];
    for (int c = 0; c < 3; c++) { wantRec[c].resize((size_t)(w >> (c ? 1 : 0)) * (h >> (c ? 1 : 0))); rdbuf(wantRec[c].data(), wantRec[c].size() * 2); }
    const bool inter = sliceType == HM_P_SLICE || sliceType == HM_B_SLICE;
    if (inter && nInter++ == maxInter) break;
    nS++;
    FrameBuf fb; hostsim_alloc_frame(fb, P);
    fseek(fy, (long)(frameBytes * poc), SEEK_SET);
    if (!hostsim_read_yuv(fy, fb, P)) return 3;
    if (inter) {
      fb.imeta = (InterMeta *)calloc(nctu, sizeof(InterMeta)); fb.intMv = (MvD *)calloc((size_t)nctu * 32, sizeof(MvD));
      InterPic *ip = (InterPic *)calloc(1, sizeof(InterPic)); fb.ip = ip;
      ip->sliceType = sliceType; ip->poc = poc; ip->numRefIdx[0] = numRef[0]; ip->numRefIdx[1] = numRef[1];
      ip->colFromL0 = misc[0]; ip->colRefIdx = misc[1]; ip->tmvp = misc[2]; ip->mvdL1Zero = misc[3]; ip->maxMergeCand = misc[4]; ip->checkLDC = misc[5]; ip->cabacInitType = misc[6];
      ip->lambdaMotionSAD = lmSAD; ip->lambdaMotionSSE = lmSSE;
      for (int l = 0; l < 2; l++) for (int i = 0; i < numRef[l]; i++) {
        FinalPic &f = finals[refPoc[l][i]]; RefPicDev &r = ip->ref[l][i];
        for (int c = 0; c < 3; c++) { const int mg = HM_REF_MARGIN >> (c ? 1 : 0); r.plane[c] = f.buf[c].data() + (size_t)mg * f.stride[c] + mg; r.stride[c] = f.stride[c]; }
        r.poc = f.poc; r.isLongTerm = refLT[l][i]; r.predMode = f.pm.data();
        for (int ll = 0; ll < 2; ll++) { r.mv[ll] = f.mv[ll].data(); r.refIdx[ll] = f.ri[ll].data(); memcpy(r.refPoc[ll], f.refPoc[ll], sizeof(r.refPoc[ll])); memcpy(r.refLT[ll], f.refLT[ll], sizeof(r.refLT[ll])); }
      }
      for (int i1 = 0; i1 < numRef[1]; i1++) { ip->list1ToList0[i1] = -1; for (int i0 = 0; i0 < numRef[0]; i0++) if (refPoc[0][i0] == refPoc[1][i1]) { ip->list1ToList0[i1] = i0; break; } }
    }
    hm355_fill_slice_params(&fb, bd, qp, lambda, wcb);
    P.frames = &fb;
    // the CTUs in the order the library's work list holds them: step by step, the slices of a step one after the other
    std::vector<WorkItem> items; std::vector<int> stepStart;
    hm355_build_schedule(P.wCtu, P.hCtu, 0, 1, items, stepStart, 0, 0, 0, -1, NULL, inter, w, h, P.slice ? &slices : NULL);
    if ((int)items.size() != nctu) { fprintf(stderr, "the schedule holds %zu CTUs of %d\n", items.size(), nctu); return 4; }
    for (size_t i = 0; i < items.size(); i++) process_ctu(&sh, &P, &items[i], 0);
    int slcBad = 0;
    for (int a = 0; a < nctu; a++) {
      const char *what = 0;
      if (!inter) memcpy(fb.meta[a].pred, wantMeta[a].pred, 256);   // (an I picture's dump carries compressMotion's prediction modes: every CU is intra either way)
      if (fb.stat[a].cost != wantStat[a].cost || fb.stat[a].bits != wantStat[a].bits || fb.stat[a].dist != wantStat[a].dist) what = "cost/bits/dist";
      else if (memcmp(&fb.meta[a], &wantMeta[a], sizeof(CtuMeta))) what = "decision arrays";
      else if (inter && memcmp(&fb.imeta[a], &wantIm[a], sizeof(InterMeta))) what = "motion arrays";
      else if (memcmp(fb.coef + (size_t)a * HM_COEF_CTU, &wantCoef[(size_t)a * HM_COEF_CTU], HM_COEF_CTU * 4)) what = "coefficients";
      if (what) { slcBad++; if (slcBad <= 3) printf("POC %d CTU %d: %s differ (got %.1f/%u/%u want %.1f/%u/%u)\n", poc, a, what, fb.stat[a].cost, fb.stat[a].bits, fb.stat[a].dist, wantStat[a].cost, wantStat[a].bits, wantStat[a].dist); }
    }
    for (int c = 0; c < 3; c++) {
      const int pw = w >> (c ? 1 : 0), ph = h >> (c ? 1 : 0);
      for (int y = 0; y < ph; y++) for (int x = 0; x < pw; x++) if ((uint16_t)fb.rec[c][y * P.stride[c] + x] != wantRec[c][(size_t)y * pw + x]) { slcBad++; y = ph; break; }
    }
    printf("POC %d: %s\n", poc, slcBad ? "MISMATCH" : "ok");
    bad += slcBad;
  }
  printf("%d pictures, %d slices, %s\n", nS, slices.count(), bad ? "MISMATCH" : "all bit-exact");
  return bad ? 1 : 0;
}
