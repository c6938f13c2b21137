// hm355 -- candidates in lanes, 8x8 blocks: where a batch of 8x8 blocks keeps its data (Simt<3>), and the chroma of a 16x16 CU.  An 8x8
// luma prediction unit has at most 11 RD candidates (8 by SATD + up to 3 most probable modes), so its first pass
// (simt_luma_first_pass<3>, hm355_simt.h) always runs as one batch with every candidate in a slot of its own.  The serial chains, the
// sample passes and the first pass itself are those of hm355_simt.h at L2 = 3.  Included from hm355_core.h after hm355_simt4.h.
#pragma once

#define HM_S8 11                          // candidates per batch: 8 by SATD + up to 3 most probable modes
struct Simt8A {                           // overlays Shared::bufA
  int32_t tile[2][64];                    // transform stages of the candidate under the lanes
  int32_t tab[SimtDim<3>::T_N];           // bit costs of the start state
  double outCost[HM_S8];
  uint32_t outDist[HM_S8], outFrac[HM_S8];
  int16_t cs[64][HM_S8];                  // coefficients in scan order
  uint8_t ctx[SimtDim<3>::NCTX][HM_S8];   // context states of each candidate
  uint8_t outCbf[HM_S8], best;            // best: the winning chroma mode's index
  uint8_t lps[128];
};
struct Simt8B {                           // overlays Shared::u behind the reference sample lines
  int32_t dc[64][HM_S8];                  // level at decision time (low half) | final signed level (high half), scan order
  uint8_t scan[3][64];                    // scan position -> raster position
  uint8_t scanCG[3][4];
};
static_assert(sizeof(Simt8A) <= sizeof(((Shared *)0)->bufA), "Simt8A overlays bufA");
static_assert(offsetof(RefLds, refMain) + sizeof(Simt8B) <= sizeof(((Shared *)0)->u), "Simt8B overlays the tail of the LDS union");
static_assert(HM_INTRA_FAST_8x8 + HM_NUM_MPM <= HM_S8 && HM_S8 <= sizeof(((Shared *)0)->rdModeList) / sizeof(int32_t), "the longest candidate list of an 8x8 PU (est_intra_pred_qt) fits one batch");
template <> struct Simt<3> {              // a batch of 8x8 blocks: RDOQ prices a decided level again, the significance increments are computed
  enum { JOBS = HM_S8, KEEPS_COST = 0, TS = 8, ONE_BATCH = 1 };      // TS: row of the transform tile; ONE_BATCH: every candidate list fits one batch
  Simt8A *A; Simt8B *B;
  HM_FINL_M explicit Simt(Shared *e) : A((Simt8A *)e->bufA), B((Simt8B *)((char *)&e->u + offsetof(RefLds, refMain))) {}
  HM_FINL_M int32_t *tile(int stage) const { return A->tile[stage]; }
  HM_FINL_M uint8_t &out_cbf(int k) const { return A->outCbf[k]; }
  HM_FINL_M uint32_t &out_dist(int k) const { return A->outDist[k]; }
  HM_FINL_M uint32_t &out_frac(int k) const { return A->outFrac[k]; }
  HM_FINL_M double &out_cost(int k) const { return A->outCost[k]; }
  HM_FINL_M int luma_scan(int mode) const { return intra_scan_type(mode); }   // getCoefScanIdx: mode-dependent up to 8x8
  HM_FINL_M int32_t *tab() const { return A->tab; }
  HM_FINL_M uint8_t &ctx(int c, int k) const { return A->ctx[c][k]; }
  HM_FINL_M uint8_t *lps() const { return A->lps; }
  HM_FINL_M int scan_pos(int scanType, int sp) const { return B->scan[scanType][sp]; }
  // B->dc: level at decision time in the low half, the final signed level in the high half, bit 30 marks a group RDOQ zeroed
  HM_FINL_M void put_dec(int sp, int k, uint32_t level) const { B->dc[sp][k] = (int32_t)level; }
  HM_FINL_M void mark_zeroed(int sp, int k) const { B->dc[sp][k] |= 0x40000000; }
  HM_FINL_M int dec(int sp, int k) const { return B->dc[sp][k] & 0xffff; }
  HM_FINL_M int zeroed(int sp, int k) const { return B->dc[sp][k] & 0x40000000; }
  HM_FINL_M void put_lev(int sp, int k, int v) const { B->dc[sp][k] = (B->dc[sp][k] & 0xffff) | (int32_t)((uint32_t)v << 16); }
  HM_FINL_M int lev(int sp, int k) const { return B->dc[sp][k] >> 16; }
  HM_FINL_M int cs(int sp, int k) const { return A->cs[sp][k]; }
  HM_FINL_M int cg_pos(int scanType, int cg) const { return B->scanCG[scanType][cg]; }
  HM_FINL_M int sig_inc(int scanType, int firstCtx, int pattern, int sp, int chroma) const { return sig_ctx_inc(pattern, firstCtx, B->scan[scanType][sp], 3, chroma); }
  HM_FINL_M void keep_cost(int, int, double) const {}
  HM_FINL_M double cost_at(int, int) const { return 0; }
  HM_FINL_M void load_scans(const Shared *e) const
  {
    HM_PAR_FOR(i, 192) { const int ty = i >> 6, sp = i & 63; B->scan[ty][sp] = (uint8_t)e->tab->scan[ty][1][sp]; }
    HM_PAR_FOR(i, 12) { const int ty = i >> 2, cg = i & 3; B->scanCG[ty][cg] = (uint8_t)e->tab->scanCG[ty][1][cg]; }
  }
};
typedef Simt<3> Simt8;

// ------------------------------------------------------------------------------------------------
// chroma of a 16x16 CU whose luma transform is not split: one 8x8 block per component under the five chroma modes
// (estIntraPredChromaQT :2698-2849), ten evaluations from the CU's entry snapshot: sample work job after job on the 64 lanes, the RDOQ
// chains one job per lane (job = 2 * modeIndex + component - 1), then one lane per mode counts the mode's bits and the modes are
// compared in the reference's order (simt_pick_chroma_mode, hm355_simt.h).  An 8x8 chroma block
// never tries transform skip and always scans diagonally.  Writes the winner (dirC / cbf / ts of the CU, coefficients, reconstruction
// into ws->reco) and returns its distortion.
// ------------------------------------------------------------------------------------------------
HM_FINL int s8_pred_sample_chroma(const Shared *e, int rs, int mode, int x, int y, int dcVal)
{ // an 8x8 chroma block: no edge filters, unfiltered reference lines of slot rs
  return intra_pred_sample(e->u.ref.refTop[rs], e->u.ref.refLeft[rs], 8, 3, 0, mode, x, y, dcVal, 0);
}
HM_DEV HM_NOINLINE uint32_t simt8_chroma_cu16(Shared *e, int cuZ)
{
  HM_ENTRY(e); cuZ = HM_UNI(cuZ);
  CtuMeta *m = (&e->meta); WorkSpace *ws = e->ws;
  const TU t = tu_root(e, cuZ, 2);
  const int r = hm_z2r(cuZ), bitDepth = e->bitDepth;
  const int x4 = e->ctuX * 16 + (r & 15), y4 = e->ctuY * 16 + (r >> 4), px = e->ctuX * 32 + t.cx, py = e->ctuY * 32 + t.cy;
  simt_chroma_ref_lines(e, px, py, 8, x4, y4);
  int modeList[5];
  const int lumaDir = m->dirL[cuZ];
  allowed_chroma_dirs(lumaDir, modeList);
  const Simt8 S(e); Simt8A *A = S.A;
  simt_setup(e, S, &e->cur, 10, 1, 5, 5, C_CHROMA_PRED);             // chroma cbf at the CU's root TU: context 5 + transform depth 0
  const SimtPar p = simt_params<3>(e, 1);
  const uint32_t baseFrac = (uint32_t)(e->cur.frac & 32767);
  const int dcVal[2] = { ref_dc_val(e, 0, 8), ref_dc_val(e, 1, 8) };
  const int shiftSse = (bitDepth - 8) << 1;
  // ---- residual + forward transform of every job
  for (int job = 0; job < 10; job++) {
    const int c = job & 1, dirC = modeList[job >> 1], mode = dirC == DM_CHROMA_IDX ? lumaDir : dirC, ps = e->stride[1 + c];
    simt_residual_fwd(S, e->fb.org[1 + c] + (size_t)py * ps + px, ps, bitDepth, SCAN_DIAG, job,
                      [&](int x, int y) HM_LAMBDA_INL { return s8_pred_sample_chroma(e, c, mode, x, y, dcVal[c]); });
  }
  HM_WAVE_FOR(k) { if (k < 10) A->outCbf[k] = (uint8_t)(simt_rdoq(S, p, k, SCAN_DIAG) > 0); }
  HM_SYNC();
  // ---- reconstruction + distortion of a job (also used for the winner's reconstruction afterwards)
  for (int pass = 0; pass < 12; pass++) {
    int job = pass;
    if (pass == 10) {                                                // all costs are in: bits and decision, then the winner's two jobs once more
      const int best = simt_pick_chroma_mode(e, S, baseFrac, modeList, [&](int k, int src, uint32_t *frac) HM_LAMBDA_INL { simt_code_coeff(e, S, k, src, 1, SCAN_DIAG, frac); });
      if (hm_lane() == 0) A->best = (uint8_t)best;
      HM_SYNC();
    }
    const int best = pass >= 10 ? A->best : 0;
    if (pass >= 10) job = 2 * best + (pass - 10);
    const int c = job & 1, dirC = modeList[job >> 1], mode = dirC == DM_CHROMA_IDX ? lumaDir : dirC, ps = e->stride[1 + c], cbf = A->outCbf[job];
    const Pel *org = e->fb.org[1 + c] + (size_t)py * ps + px;
    const int po = HM_PLANE_OFF(1 + c);
    // the winner: reconstruction and levels to where the CU's data lives
    simt_dequant_inv1(S, p, SCAN_DIAG, job, cbf, pass >= 10 ? e->cc + po + t.cOff : (TCoeff *)0);
    uint32_t sse = 0;
    simt_inv2_recon(S, bitDepth, cbf, [&](int x, int y) HM_LAMBDA_INL { return s8_pred_sample_chroma(e, c, mode, x, y, dcVal[c]); },
                    [&](int x, int y, int rr) HM_LAMBDA_INL {
                      const int d = org[y * ps + x] - rr; sse += (uint32_t)((d * d) >> shiftSse);
                      if (pass >= 10) ws->reco[po + (t.cy + y) * 32 + t.cx + x] = (Pel)rr;
                    });
    const uint32_t dsum = hm_wave_sum(sse);
    if (pass < 10 && hm_lane() == 0) A->outDist[job] = (uint32_t)(e->fb.chromaWeight * (double)dsum);   // getDistPart, TComRdCost.cpp:447-450
    HM_SYNC();
  }
  const int best = A->best, cbfU = A->outCbf[2 * best], cbfV = A->outCbf[2 * best + 1];
  const uint32_t bestDist = A->outDist[2 * best] + A->outDist[2 * best + 1];
  const int bm = modeList[best];
  HM_PAR_FOR(i, 16) { m->cbf[1][cuZ + i] = (uint8_t)cbfU; m->cbf[2][cuZ + i] = (uint8_t)cbfV; m->ts[1][cuZ + i] = 0; m->ts[2][cuZ + i] = 0; m->dirC[cuZ + i] = (uint8_t)bm; }
  simt_store_chroma_mode(S, 2 * best, &e->cur, A->outFrac[2 * best]);          // e->cur: the estimator after the winning mode's count
  HM_SYNC();
  return bestDist;
}
