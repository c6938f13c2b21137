// hm355 -- candidates in lanes, 8x8 blocks: the first pass of estIntraPredQT (:2473-2490) over the RD candidates of an 8x8
// luma prediction unit.  Every candidate is the same evaluation of one 8x8 transform block from the same CABAC snapshot
// (xRecurIntraCodingQT with bCheckFirst: no split), and only its cost is kept -- the winner is evaluated again by the closing
// pass with the full residual quadtree.  So the wavefront alternates between two shapes of parallelism:
//   * sample work (prediction, residual, 8-point transforms, de-quantisation, reconstruction, SSE) one candidate after the
//     other with the 64 lanes on the block's 64 samples,
//   * the serial chains (RDOQ level decision, CABAC bit estimate) for all candidates at once, one candidate per lane.
// Arithmetic and operation order are the reference's throughout.  The serial chains are the per-lane coefficient coder of
// hm355_simt.h at L2 = 3; the sample passes are the three s8_* functions below.  Included from hm355_core.h after hm355_simt4.h.
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
template <> struct Simt<3> {              // a batch of 8x8 blocks: RDOQ prices a decided level again, the significance increments are computed
  enum { JOBS = HM_S8, KEEPS_COST = 0 };
  Simt8A *A; Simt8B *B;
  HM_FINL_M explicit Simt(Shared *e) : A((Simt8A *)e->bufA), B((Simt8B *)((char *)&e->u + offsetof(RefLds, refMain))) {}
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

// ---- the sample passes of one 8x8 block, the 64 lanes on its 64 samples; pred(x, y): the predicted sample
// residual + forward transform (xTrMxN :836); coefficients to A->cs[.][job] in the scan order `scanType`
template <class Pred> HM_FINL void s8_residual_fwd(const Simt8 &S, const Pel *org, int ps, int bitDepth, int scanType, int job, Pred pred)
{
  Simt8A *A = S.A;
  const int s1 = 3 + bitDepth + 6 - 15, a1 = 1 << (s1 - 1), s2 = 9, a2 = 256;
  HM_PAR_FOR(l, 64) { const int y = l >> 3, x = l & 7; A->tile[0][l] = org[y * ps + x] - pred(x, y); }
  HM_SYNC();
  HM_PAR_FOR(l, 64) { // first stage
    const int j = l >> 3, kk = l & 7; int32_t acc = 0;
    for (int i = 0; i < 8; i++) acc += HM_LT()->tmat[(kk * 4) * HM_TSTRIDE + i] * A->tile[0][j * 8 + i];
    A->tile[1][kk * 8 + j] = (acc + a1) >> s1;
  }
  HM_SYNC();
  HM_PAR_FOR(l, 64) { // second stage, one lane per scan position
    const int blkPos = S.B->scan[scanType][l], kk = blkPos >> 3, j = blkPos & 7; int32_t acc = 0;
    for (int i = 0; i < 8; i++) acc += HM_LT()->tmat[(kk * 4) * HM_TSTRIDE + i] * A->tile[1][j * 8 + i];
    A->cs[l][job] = (int16_t)((acc + a2) >> s2);
  }
  HM_SYNC();
}
// de-quantisation of job's levels into raster order + first inverse stage (xITrMxN :894); coef: where to store the levels as well, or null
HM_FINL void s8_dequant_inv1(const Simt8 &S, const SimtPar &p, int scanType, int job, int cbf, TCoeff *coef)
{
  Simt8A *A = S.A;
  if (cbf) {
    HM_PAR_FOR(l, 64) {
      const int lv = S.B->dc[l][job] >> 16, blk = S.B->scan[scanType][l];
      if (coef) coef[blk] = lv;
      A->tile[0][blk] = simt_dequant(p, lv);
    }
    HM_SYNC();
    HM_PAR_FOR(l, 64) {
      const int j = l >> 3, i = l & 7; int32_t acc = 0;
      for (int kk = 0; kk < 8; kk++) acc += HM_LT()->tmat[(kk * 4) * HM_TSTRIDE + i] * A->tile[0][kk * 8 + j];
      A->tile[1][j * 8 + i] = hm_clip3(-32768, 32767, (acc + 64) >> 7);
    }
    HM_SYNC();
  } else if (coef) { HM_PAR_FOR(l, 64) coef[l] = 0; }
}
// second inverse stage + prediction + clip: out(x, y, reconstructed sample)
template <class Pred, class Out> HM_FINL void s8_inv2_recon(const Simt8 &S, int bitDepth, int cbf, Pred pred, Out out)
{
  const int maxv = (1 << bitDepth) - 1, is2 = 20 - bitDepth;
  HM_PAR_FOR(l, 64) {
    const int j = l >> 3, i = l & 7; int resi = 0;
    if (cbf) {
      int32_t acc = 0;
      for (int kk = 0; kk < 8; kk++) acc += HM_LT()->tmat[(kk * 4) * HM_TSTRIDE + i] * S.A->tile[1][kk * 8 + j];
      resi = hm_clip3(-32768, 32767, (acc + (1 << (is2 - 1))) >> is2);
    }
    out(i, j, hm_clip3(0, maxv, pred(i, j) + resi));
  }
}

// ------------------------------------------------------------------------------------------------
// The first pass over the RD candidates e->rdModeList[0..numModes) of the 8x8 PU `tv` (a 2Nx2N CU of depth 3).  e->cur holds the
// CU's entry snapshot, e->u.ref the PU's reference samples (both the plain and the smoothed lines), e->mpmPreds its most probable
// modes.  Returns the winning mode: the candidate of least cost, the first one on a tie (estIntraPredQT :2520-2560).
// ------------------------------------------------------------------------------------------------
HM_DEV HM_NOINLINE int simt8_luma_first_pass(Shared *e, TU tv, int numModes)
{
  HM_ENTRY(e); numModes = HM_UNI(numModes); tv = hm_uni_struct(tv);
  const TU *t = &tv;
  const int ps = e->stride[0], bitDepth = e->bitDepth;
  const Simt8 S(e); Simt8A *A = S.A;
  uint32_t commonFrac;                                             // bins every candidate codes alike (xEncIntraHeader :965, xEncSubdivCbfQT :856)
  {
    CabacR r; cabr_load(e, r, &e->cur);
    r.frac &= 32767;
    if (e->im) { code_skip_flag(e, &r, t->cuZ); enc_bin(e, &r, C_PRED_MODE, 1); }
    enc_bin(e, &r, C_PART, 1);                                     // 2Nx2N at the smallest CU size
    enc_bin(e, &r, C_SUBDIV + 2, 0);                               // transform_split of the 8x8 root TU: not split in this pass
    commonFrac = (uint32_t)r.frac;
  }
  simt_setup(e, S, &e->cur, numModes, 0, 1, 1, C_INTRA_LUMA);       // luma cbf at the CU's root TU: context 1
  const SimtPar p = simt_params<3>(e, 0);
  const Pel *org = e->fb.org[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
  const int dcVal = ref_dc_val(e, 0, 8);
  // ---- residual + forward transform of every candidate, lanes on the samples; coefficients to A->cs in the candidate's scan order
  for (int c = 0; c < numModes; c++) {
    const int mode = e->rdModeList[c];
    s8_residual_fwd(S, org, ps, bitDepth, intra_scan_type(mode), c, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, 8, 3, x, y, dcVal, bitDepth); });
  }
  // ---- level decision of every candidate, one per lane
  HM_WAVE_FOR(k) {
    if (k < numModes) A->outCbf[k] = (uint8_t)(simt_rdoq(S, p, k, intra_scan_type(e->rdModeList[k])) > 0);
  }
  HM_SYNC();
  // ---- reconstruction + distortion of every candidate, lanes on the samples
  const int shiftSse = (bitDepth - 8) << 1;
  for (int c = 0; c < numModes; c++) {
    const int mode = e->rdModeList[c], cbf = A->outCbf[c];
    s8_dequant_inv1(S, p, intra_scan_type(mode), c, cbf, (TCoeff *)0);
    uint32_t sse = 0;
    s8_inv2_recon(S, bitDepth, cbf, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, 8, 3, x, y, dcVal, bitDepth); },
                  [&](int x, int y, int r) HM_LAMBDA_INL { const int d = org[y * ps + x] - r; sse += (uint32_t)((d * d) >> shiftSse); });
    const uint32_t dist = hm_wave_sum(sse);
    if (hm_lane() == 0) A->outDist[c] = dist;
    HM_SYNC();
  }
  // ---- bits and cost of every candidate, one per lane (xGetIntraBitsQT :1038)
  HM_WAVE_FOR(k) {
    if (k < numModes) {
      const int mode = e->rdModeList[k], cbf = A->outCbf[k];
      uint32_t frac = commonFrac;
      simt_luma_mode_bits(e, S, k, &frac, mode);
      simt_bin(e, S, k, &frac, SimtDim<3>::X_CBF, cbf);
      if (cbf) simt_code_coeff(e, S, k, k, 0, intra_scan_type(mode), &frac);
      A->outFrac[k] = frac;
      A->outCost[k] = calc_rd_cost(e, frac >> 15, A->outDist[k]);
    }
  }
  HM_SYNC();
  double bestCost = HM_MAX_DOUBLE; int best = 0;
  for (int c = 0; c < numModes; c++) { const double v = A->outCost[c]; if (v < bestCost) { bestCost = v; best = c; } }
  best = HM_UNI(best);
  const int bestMode = e->rdModeList[best];
  e->s8Winner = best | (best << 8);                                // slot and place in the list: simt_luma_winner_as_single_tu (hm355_simt16.h) picks the winner's evaluation up from the overlays
  HM_SYNC();
  return bestMode;
}

// ------------------------------------------------------------------------------------------------
// chroma of a 16x16 CU whose luma transform is not split: one 8x8 block per component under the five chroma modes
// (estIntraPredChromaQT :2698-2849), ten evaluations from the CU's entry snapshot: sample work job after job on the 64 lanes, the RDOQ
// chains one job per lane (job = 2 * modeIndex + component - 1), then one lane per mode counts the mode's bits (chroma prediction mode,
// both cbfs, Cb and Cr coefficients: xGetIntraBitsQT :1038) and the modes are compared in the reference's order.  An 8x8 chroma block
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
    s8_residual_fwd(S, e->fb.org[1 + c] + (size_t)py * ps + px, ps, bitDepth, SCAN_DIAG, job,
                    [&](int x, int y) HM_LAMBDA_INL { return s8_pred_sample_chroma(e, c, mode, x, y, dcVal[c]); });
  }
  HM_WAVE_FOR(k) { if (k < 10) A->outCbf[k] = (uint8_t)(simt_rdoq(S, p, k, SCAN_DIAG) > 0); }
  HM_SYNC();
  // ---- reconstruction + distortion of a job (also used for the winner's reconstruction afterwards)
  for (int pass = 0; pass < 12; pass++) {
    int job = pass;
    if (pass == 10) {                                                // all costs are in: bits and decision, then the winner's two jobs once more
      HM_WAVE_FOR(k) {
        if (k < 10 && !(k & 1)) {
          const int dirC = modeList[k >> 1];
          uint32_t frac = baseFrac;
          simt_bin(e, S, k, &frac, SimtDim<3>::X_MODE, dirC != DM_CHROMA_IDX);    // codeIntraDirChroma :692
          if (dirC != DM_CHROMA_IDX) frac += 2u * 32768u;
          const int cbfU = A->outCbf[k], cbfV = A->outCbf[k + 1];
          simt_bin(e, S, k, &frac, SimtDim<3>::X_CBF, cbfU);         // xEncSubdivCbfQT :856: both cbfs at the root TU
          simt_bin(e, S, k, &frac, SimtDim<3>::X_CBF, cbfV);
          if (cbfU) simt_code_coeff(e, S, k, k, 1, SCAN_DIAG, &frac);
          if (cbfV) simt_code_coeff(e, S, k, k + 1, 1, SCAN_DIAG, &frac);
          const uint32_t dist = A->outDist[k] + A->outDist[k + 1];
          A->outFrac[k] = frac;
          A->outCost[k] = calc_rd_cost(e, frac >> 15, dist);
        }
      }
      HM_SYNC();
      double bestCost = HM_MAX_DOUBLE; int best = 0;
      for (int mi = 0; mi < 5; mi++) { const double v = A->outCost[2 * mi]; if (v < bestCost) { bestCost = v; best = mi; } }
      best = HM_UNI(best);
      if (hm_lane() == 0) A->best = (uint8_t)best;
      HM_SYNC();
    }
    const int best = pass >= 10 ? A->best : 0;
    if (pass >= 10) job = 2 * best + (pass - 10);
    const int c = job & 1, dirC = modeList[job >> 1], mode = dirC == DM_CHROMA_IDX ? lumaDir : dirC, ps = e->stride[1 + c], cbf = A->outCbf[job];
    const Pel *org = e->fb.org[1 + c] + (size_t)py * ps + px;
    const int po = HM_PLANE_OFF(1 + c);
    // the winner: reconstruction and levels to where the CU's data lives
    s8_dequant_inv1(S, p, SCAN_DIAG, job, cbf, pass >= 10 ? e->cc + po + t.cOff : (TCoeff *)0);
    uint32_t sse = 0;
    s8_inv2_recon(S, bitDepth, cbf, [&](int x, int y) HM_LAMBDA_INL { return s8_pred_sample_chroma(e, c, mode, x, y, dcVal[c]); },
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
