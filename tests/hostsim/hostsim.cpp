// DEBUGGING AID, NOT PRODUCT: compiles hm-16.2_amd/csrc/hm355_core.h -- the very source the gfx950
// kernel is built from -- for the host with one "lane" (HM_NT == 1), so that the decision logic can be
// stepped through and diffed against the oracle in a container that has no GPU.  It is built only by
// tests/ (never linked into libhm355.so) and it cannot exercise cross-lane behaviour; the GPU parity
// tests remain the gate.  With -DHM355_HOSTSIM_REVERSE every lane-parallel loop runs backwards, which
// exposes accidental order dependences between "lanes".
//   hostsim <in.yuv> <w> <h> <bitdepth> <frames> <qp> <wpp> <dump.bin>       (same dump as oracle CLI)
#include "hostsim_common.h"

int main(int argc, char **argv)
{
  if (argc < 9) { fprintf(stderr, "usage: %s in.yuv w h bd frames qp wpp dump.bin\n", argv[0]); return 2; }
  const int w = atoi(argv[2]), h = atoi(argv[3]), bd = atoi(argv[4]), frames = atoi(argv[5]), qp = atoi(argv[6]), wpp = atoi(argv[7]);
  FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[8], "wb");
  if (!fi || !fo) { perror("open"); return 1; }
  Params P; hostsim_params(P, w, h, bd, wpp);
#ifdef HM355_HOSTSIM_REVERSE
  P.fewWaves = 1;     // the reversed build also takes the small-launch code path (4x4 leaves of a quadtree on one lane)
#endif
  const int nctu = P.wCtu * P.hCtu;
  std::vector<FrameBuf> fbs(frames);
  double lambda, cw; hm355_intra_lambda(qp, &lambda, &cw);
  for (int f = 0; f < frames; f++) {
    hostsim_alloc_frame(fbs[f], P);
    if (!hostsim_read_yuv(fi, fbs[f], P)) return 3;
    hm355_fill_slice_params(&fbs[f], bd, qp, lambda, cw);
  }
  P.frames = fbs.data();
  std::vector<WorkItem> items; std::vector<int> stepStart;
  hm355_build_schedule(P.wCtu, P.hCtu, wpp, frames, items, stepStart);
  static Shared sh;
  if (getenv("HM355_DIRTY")) {
    // debugging aid: everything the search writes before it reads may hold anything -- fill the workspace, the LDS state, the reconstruction, the decision /
    // coefficient / statistics arrays and the CABAC hand-off states with noise; the result must not change (tests/test_host_logic.py)
    unsigned long long x = 88172645463325252ull ^ (unsigned long long)atoll(getenv("HM355_DIRTY"));
    auto fill = [&](void *p, size_t n) { unsigned char *b = (unsigned char *)p; for (size_t i = 0; i < n; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b[i] = (unsigned char)(x >> 24); } };
    fill(P.ws, sizeof(WorkSpace)); fill(&sh, sizeof(sh));
    for (int f = 0; f < frames; f++) {
      FrameBuf &fb = fbs[f];
      for (int c = 0; c < 3; c++) fill(fb.rec[c], hostsim_plane_samples(P, c) * sizeof(Pel));
      fill(fb.meta, nctu * sizeof(CtuMeta)); fill(fb.coef, (size_t)nctu * HM_COEF_CTU * sizeof(TCoeff)); fill(fb.stat, nctu * sizeof(CtuStat)); fill(fb.endState, nctu * sizeof(Cabac));
    }
  }
  for (size_t i = 0; i < items.size(); i++) process_ctu(&sh, &P, &items[i], 0);
  hostsim_write_hmd1_header(fo, P, frames);
  for (int f = 0; f < frames; f++) hostsim_write_hmd1_picture(fo, P, fbs[f], f);
  fclose(fo); fclose(fi);
  return 0;
}
