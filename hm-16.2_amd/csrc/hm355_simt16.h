// hm355 -- candidates in lanes, 16x16 blocks: where a batch of 16x16 blocks keeps its data (Simt<4>).  The first pass over the RD candidates
// of a 16x16 luma prediction unit (a 2Nx2N CU of depth 2) is simt_luma_first_pass<4> of hm355_simt.h, its serial chains and sample passes
// those of hm355_simt.h at L2 = 4.
// A candidate needs 256 x (coefficient + level at decision time + final level) in 16-bit lane-indexed columns, so the two LDS overlays of
// the smaller batches hold HM_S16 = 4 of them with the transform tile lying over the decision-time column (the tile is idle during the
// chains; that column is written by RDOQ and dead once RDOQ returns).  A PU has 3 to 6 candidates, so one with more than four takes a second
// batch (Simt<4>::ONE_BATCH == 0).  The 16x16 scan is composed from the scan of the 4x4 grid of coefficient groups and the scan inside a group.
// Included from hm355_core.h after hm355_simt8.h.
#pragma once

#define HM_S16 4                          // candidates (lanes in use) per batch
#define HM_S16T 17                        // padded row of the transform tile: both transform passes free of bank conflicts
struct Simt16A {                          // overlays Shared::bufA
  union {
    int32_t tile[2][16 * HM_S16T];        // transform stages of the candidate under the lanes
    uint16_t dec[256][HM_S16];            // RDOQ: level at decision time, bit 15: the group was zeroed afterwards
  };
  int16_t cs[256][HM_S16];                // coefficients in scan order
};
struct Simt16B {                          // overlays Shared::u behind the reference sample lines
  int16_t lev[256][HM_S16];               // final signed levels, scan order
  int32_t tab[SimtDim<4>::T_N];           // bit costs of the start state
  double outCost[HM_S16];
  uint32_t outDist[HM_S16], outFrac[HM_S16];
  uint8_t ctx[SimtDim<4>::NCTX][HM_S16];  // context states of each candidate
  uint8_t outCbf[HM_S16];
  uint8_t scanCG[16], scanIn[16];         // diagonal scan (the only one a 16x16 block uses), scan position -> raster position: of a coefficient group in the 4x4 grid of groups, of a coefficient in its group
  uint8_t lps[128];
};
static_assert(sizeof(Simt16A) <= sizeof(((Shared *)0)->bufA), "Simt16A overlays bufA");
static_assert(offsetof(RefLds, refMain) + sizeof(Simt16B) <= sizeof(((Shared *)0)->u), "Simt16B overlays the tail of the LDS union");
static_assert(sizeof(((Simt16A *)0)->dec) <= sizeof(((Simt16A *)0)->tile) && offsetof(Simt16B, outCost) % 8 == 0, "the decision-time column lies under the tile");
template <> struct Simt<4> {              // a batch of 16x16 blocks: 16-bit columns, RDOQ prices a decided level again, the scan and the significance increments are computed
  enum { JOBS = HM_S16, KEEPS_COST = 0, TS = HM_S16T, ONE_BATCH = 0 };    // TS: row of the transform tile; ONE_BATCH: a PU with more than four candidates takes a second batch
  Simt16A *A; Simt16B *B;
  HM_FINL_M explicit Simt(Shared *e) : A((Simt16A *)e->bufA), B((Simt16B *)((char *)&e->u + offsetof(RefLds, refMain))) {}
  HM_FINL_M int32_t *tile(int stage) const { return A->tile[stage]; }
  HM_FINL_M uint8_t &out_cbf(int k) const { return B->outCbf[k]; }
  HM_FINL_M uint32_t &out_dist(int k) const { return B->outDist[k]; }
  HM_FINL_M uint32_t &out_frac(int k) const { return B->outFrac[k]; }
  HM_FINL_M double &out_cost(int k) const { return B->outCost[k]; }
  HM_FINL_M int luma_scan(int) const { return SCAN_DIAG; }            // getCoefScanIdx: a 16x16 block scans diagonally whatever its mode
  HM_FINL_M int32_t *tab() const { return B->tab; }
  HM_FINL_M uint8_t &ctx(int c, int k) const { return B->ctx[c][k]; }
  HM_FINL_M uint8_t *lps() const { return B->lps; }
  HM_FINL_M int scan_pos(int, int sp) const
  {
    const int cg = B->scanCG[sp >> 4], in = B->scanIn[sp & 15];
    return ((cg >> 2) * 4 + (in >> 2)) * 16 + (cg & 3) * 4 + (in & 3);
  }
  HM_FINL_M void put_dec(int sp, int k, uint32_t level) const { A->dec[sp][k] = (uint16_t)level; }        // a level is at most 32767
  HM_FINL_M void mark_zeroed(int sp, int k) const { A->dec[sp][k] |= 0x8000; }
  HM_FINL_M int dec(int sp, int k) const { return A->dec[sp][k] & 0x7fff; }
  HM_FINL_M int zeroed(int sp, int k) const { return A->dec[sp][k] & 0x8000; }
  HM_FINL_M void put_lev(int sp, int k, int v) const { B->lev[sp][k] = (int16_t)v; }
  HM_FINL_M int lev(int sp, int k) const { return B->lev[sp][k]; }
  HM_FINL_M int cs(int sp, int k) const { return A->cs[sp][k]; }
  HM_FINL_M int cg_pos(int, int cg) const { return B->scanCG[cg]; }
  HM_FINL_M int sig_inc(int scanType, int firstCtx, int pattern, int sp, int chroma) const { return sig_ctx_inc(pattern, firstCtx, scan_pos(scanType, sp), 4, chroma); }
  HM_FINL_M void keep_cost(int, int, double) const {}
  HM_FINL_M double cost_at(int, int) const { return 0; }
  HM_FINL_M void load_scans(const Shared *e) const
  {
    HM_PAR_FOR(q, 16) { B->scanCG[q] = (uint8_t)e->tab->scanCG[SCAN_DIAG][2][q]; B->scanIn[q] = (uint8_t)e->tab->scan[SCAN_DIAG][0][q]; }
#ifdef HM355_HOSTSIM
    static int checked;                   // once: the composed scan must equal the generated table
    if (!checked) { checked = 1; for (int i = 0; i < 256; i++) if (scan_pos(SCAN_DIAG, i) != e->tab->scan[SCAN_DIAG][2][i]) abort(); }
#endif
  }
};
typedef Simt<4> Simt16;
