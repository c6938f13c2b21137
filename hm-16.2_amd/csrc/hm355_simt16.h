// hm355 -- candidates in lanes, 16x16 blocks: the first pass of estIntraPredQT (:2473-2490) over the RD candidates of a 16x16
// luma prediction unit (a 2Nx2N CU of depth 2), in the shape of the 8x8 pass of hm355_simt8.h: every candidate is the same
// evaluation of one unsplit 16x16 transform block from the same CABAC snapshot, and only its cost is kept.
//   * sample work (prediction, residual, 16-point transforms, de-quantisation, reconstruction, SSE) one candidate after the
//     other with the 64 lanes on the block's 256 samples, the prediction taken straight from the reference lines,
//   * the serial chains (RDOQ level decision, CABAC bit estimate) one candidate per lane: the per-lane coefficient coder of
//     hm355_simt.h at L2 = 4.
// A candidate needs 256 x (coefficient + level at decision time + final level) in 16-bit lane-indexed columns, so the two LDS overlays of
// the smaller batches hold HM_S16 = 4 of them with the transform tile lying over the decision-time column (the tile is idle during the
// chains; that column is written by RDOQ and dead once RDOQ returns).  A PU with more candidates runs in batches, in list order: the best
// candidate so far stays in its slot (its levels, contexts and results are what the closing pass picks up) and the next three take the
// other slots.  The 16x16 scan is composed from the scan of the 4x4 grid of coefficient groups and the scan inside a group.
// Arithmetic and operation order are the reference's throughout.  Included from hm355_core.h after hm355_simt8.h.
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
  enum { JOBS = HM_S16, KEEPS_COST = 0 };
  Simt16A *A; Simt16B *B;
  HM_FINL_M explicit Simt(Shared *e) : A((Simt16A *)e->bufA), B((Simt16B *)((char *)&e->u + offsetof(RefLds, refMain))) {}
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

#ifdef HM355_HOSTSIM
// host twin only: how many candidates the 16x16 first passes had and how many batches they took (printed at exit when HM355_S16_STATS is set)
#include <stdio.h>
struct Simt16Stats {
  unsigned long cand[8], batches[4];
  ~Simt16Stats()
  {
    if (!getenv("HM355_S16_STATS")) return;
    fprintf(stderr, "s16 candidates"); for (int i = 0; i < 8; i++) fprintf(stderr, " %lu", cand[i]);
    fprintf(stderr, "\ns16 batches"); for (int i = 0; i < 4; i++) fprintf(stderr, " %lu", batches[i]);
    fprintf(stderr, "\n");
  }
};
static Simt16Stats g_s16_stats;
#endif

// ---- the sample passes of one 16x16 block, the 64 lanes on its 256 samples; pred(x, y): the predicted sample.  The 16-point transforms are
// the plain matrix products (rows 2k of the 32-point matrix): sums of exact integer products, so they give partialButterfly16's integers.
// residual + forward transform (xTrMxN :836); coefficients to A->cs[.][job] in scan order (a 16x16 block scans diagonally)
template <class Pred> HM_FINL void s16_residual_fwd(const Simt16 &S, const Pel *org, int ps, int bitDepth, int job, Pred pred)
{
  Simt16A *A = S.A;
  const int s1 = 4 + bitDepth + 6 - 15, a1 = 1 << (s1 - 1), s2 = 10, a2 = 512;
  HM_PAR_FOR(l, 256) { const int y = l >> 4, x = l & 15; A->tile[0][y * HM_S16T + x] = org[y * ps + x] - pred(x, y); }
  HM_SYNC();
  HM_PAR_FOR(l, 256) { // first stage
    const int j = l >> 4, kk = l & 15; int32_t acc = 0;
    for (int i = 0; i < 16; i++) acc += HM_LT()->tmat[(kk * 2) * HM_TSTRIDE + i] * A->tile[0][j * HM_S16T + i];
    A->tile[1][kk * HM_S16T + j] = (acc + a1) >> s1;
  }
  HM_SYNC();
  HM_PAR_FOR(l, 256) { // second stage, one lane per scan position
    const int blkPos = S.scan_pos(SCAN_DIAG, l), kk = blkPos >> 4, j = blkPos & 15; int32_t acc = 0;
    for (int i = 0; i < 16; i++) acc += HM_LT()->tmat[(kk * 2) * HM_TSTRIDE + i] * A->tile[1][j * HM_S16T + i];
    A->cs[l][job] = (int16_t)((acc + a2) >> s2);
  }
  HM_SYNC();
}
// de-quantisation of job's levels into raster order + first inverse stage (xITrMxN :894); coef: where to store the levels as well, or null
HM_FINL void s16_dequant_inv1(const Simt16 &S, const SimtPar &p, int job, int cbf, TCoeff *coef)
{
  Simt16A *A = S.A;
  if (cbf) {
    HM_PAR_FOR(l, 256) {
      const int lv = S.lev(l, job), blk = S.scan_pos(SCAN_DIAG, l);
      if (coef) coef[blk] = lv;
      A->tile[0][(blk >> 4) * HM_S16T + (blk & 15)] = simt_dequant(p, lv);
    }
    HM_SYNC();
    HM_PAR_FOR(l, 256) {
      const int j = l >> 4, i = l & 15; int32_t acc = 0;
      for (int kk = 0; kk < 16; kk++) acc += HM_LT()->tmat[(kk * 2) * HM_TSTRIDE + i] * A->tile[0][kk * HM_S16T + j];
      A->tile[1][j * HM_S16T + i] = hm_clip3(-32768, 32767, (acc + 64) >> 7);
    }
    HM_SYNC();
  } else if (coef) { HM_PAR_FOR(l, 256) coef[l] = 0; }
}
// second inverse stage + prediction + clip: out(x, y, reconstructed sample)
template <class Pred, class Out> HM_FINL void s16_inv2_recon(const Simt16 &S, int bitDepth, int cbf, Pred pred, Out out)
{
  const int maxv = (1 << bitDepth) - 1, is2 = 20 - bitDepth;
  HM_PAR_FOR(l, 256) {
    const int j = l >> 4, i = l & 15; int resi = 0;
    if (cbf) {
      int32_t acc = 0;
      for (int kk = 0; kk < 16; kk++) acc += HM_LT()->tmat[(kk * 2) * HM_TSTRIDE + i] * S.A->tile[1][kk * HM_S16T + j];
      resi = hm_clip3(-32768, 32767, (acc + (1 << (is2 - 1))) >> is2);
    }
    out(i, j, hm_clip3(0, maxv, pred(i, j) + resi));
  }
}
// the same passes by the batch's type, for what is written once for both sizes
HM_FINL void sn_dequant_inv1(const Simt8 &S, const SimtPar &p, int job, int cbf, TCoeff *coef, int scanType) { s8_dequant_inv1(S, p, scanType, job, cbf, coef); }
HM_FINL void sn_dequant_inv1(const Simt16 &S, const SimtPar &p, int job, int cbf, TCoeff *coef, int) { s16_dequant_inv1(S, p, job, cbf, coef); }
template <class Pred, class Out> HM_FINL void sn_inv2_recon(const Simt8 &S, int bitDepth, int cbf, Pred pred, Out out) { s8_inv2_recon(S, bitDepth, cbf, pred, out); }
template <class Pred, class Out> HM_FINL void sn_inv2_recon(const Simt16 &S, int bitDepth, int cbf, Pred pred, Out out) { s16_inv2_recon(S, bitDepth, cbf, pred, out); }
HM_FINL uint8_t *sn_out_cbf(const Simt8 &S) { return S.A->outCbf; }
HM_FINL uint8_t *sn_out_cbf(const Simt16 &S) { return S.B->outCbf; }
HM_FINL uint32_t *sn_out_dist(const Simt8 &S) { return S.A->outDist; }
HM_FINL uint32_t *sn_out_dist(const Simt16 &S) { return S.B->outDist; }
HM_FINL uint32_t *sn_out_frac(const Simt8 &S) { return S.A->outFrac; }
HM_FINL uint32_t *sn_out_frac(const Simt16 &S) { return S.B->outFrac; }

// ------------------------------------------------------------------------------------------------
// The first pass over the RD candidates e->rdModeList[0..numModes) of the 16x16 PU `tv`.  e->cur holds the CU's entry snapshot, e->u.ref
// the PU's reference samples (both the plain and the smoothed lines), e->mpmPreds its most probable modes.  Returns the winning mode: the
// candidate of least cost, the first one on a tie (estIntraPredQT :2520-2560); e->s8Winner: its slot and its place in the list.
// ------------------------------------------------------------------------------------------------
HM_DEV HM_NOINLINE int simt16_luma_first_pass(Shared *e, TU tv, int numModes)
{
  HM_ENTRY(e); numModes = HM_UNI(numModes); tv = hm_uni_struct(tv);
  const TU *t = &tv;
  const int ps = e->stride[0], bitDepth = e->bitDepth;
  const Simt16 S(e); Simt16B *B = S.B;
  uint32_t commonFrac;                                             // bins every candidate codes alike (xEncIntraHeader :965, xEncSubdivCbfQT :856)
  {
    CabacR r; cabr_load(e, r, &e->cur);
    r.frac &= 32767;
    if (e->im) { code_skip_flag(e, &r, t->cuZ); enc_bin(e, &r, C_PRED_MODE, 1); }
    enc_bin(e, &r, C_SUBDIV + 1, 0);                               // transform_split of the 16x16 root TU: not split in this pass (no part size above the smallest CU)
    commonFrac = (uint32_t)r.frac;
  }
  simt_setup(e, S, &e->cur, numModes < HM_S16 ? numModes : HM_S16, 0, 1, 1, C_INTRA_LUMA);       // luma cbf at the CU's root TU: context 1
  const SimtPar p = simt_params<4>(e, 0);
  const Pel *org = e->fb.org[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
  const int dcVal = ref_dc_val(e, 0, 16), shiftSse = (bitDepth - 8) << 1;
  double bestCost = HM_MAX_DOUBLE; int keep = -1, best = 0;        // keep: the slot of the best candidate so far (none before the first batch)
#ifdef HM355_HOSTSIM
  int batchesRun = 0;
#endif
  for (int c0 = 0; c0 < numModes;) {
    const int room = keep < 0 ? HM_S16 : HM_S16 - 1, nb = numModes - c0 < room ? numModes - c0 : room;
    // member i of the batch (candidate c0 + i) takes slot i, stepping over the kept one
    if (keep >= 0) {                                               // fresh context copies for the slots that are used again
      HM_PAR_FOR(i, SimtDim<4>::NCTX * HM_S16) {
        const int j = i / HM_S16, k = i - j * HM_S16;
        if (k != keep) S.ctx(j, k) = e->cur.s[simt_ctx_index<4>(j, 0, 1, C_INTRA_LUMA)];
      }
      HM_SYNC();
    }
    // ---- residual + forward transform of every candidate, lanes on the samples
    for (int i = 0; i < nb; i++) {
      const int slot = i + (keep >= 0 && i >= keep), mode = HM_UNI(e->rdModeList[c0 + i]);
      s16_residual_fwd(S, org, ps, bitDepth, slot, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, 16, 4, x, y, dcVal, bitDepth); });
    }
    // ---- level decision of every candidate, one per lane
    HM_WAVE_FOR(k) {
      const int i = (keep >= 0 && k > keep) ? k - 1 : k;
      if (k < HM_S16 && k != keep && i < nb) B->outCbf[k] = (uint8_t)(simt_rdoq(S, p, k, SCAN_DIAG) > 0);
    }
    HM_SYNC();
    // ---- reconstruction + distortion of every candidate, lanes on the samples
    for (int i = 0; i < nb; i++) {
      const int slot = i + (keep >= 0 && i >= keep), mode = HM_UNI(e->rdModeList[c0 + i]), cbf = HM_UNI(B->outCbf[slot]);
      s16_dequant_inv1(S, p, slot, cbf, (TCoeff *)0);
      uint32_t sse = 0;
      s16_inv2_recon(S, bitDepth, cbf, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, 16, 4, x, y, dcVal, bitDepth); },
                     [&](int x, int y, int r) HM_LAMBDA_INL { const int d = org[y * ps + x] - r; sse += (uint32_t)((d * d) >> shiftSse); });
      const uint32_t dist = hm_wave_sum(sse);
      if (hm_lane() == 0) B->outDist[slot] = dist;
      HM_SYNC();
    }
    // ---- bits and cost of every candidate, one per lane (xGetIntraBitsQT :1038)
    HM_WAVE_FOR(k) {
      const int i = (keep >= 0 && k > keep) ? k - 1 : k;
      if (k < HM_S16 && k != keep && i < nb) {
        const int mode = e->rdModeList[c0 + i], cbf = B->outCbf[k];
        uint32_t frac = commonFrac;
        simt_luma_mode_bits(e, S, k, &frac, mode);
        simt_bin(e, S, k, &frac, SimtDim<4>::X_CBF, cbf);
        if (cbf) simt_code_coeff(e, S, k, k, 0, SCAN_DIAG, &frac);
        B->outFrac[k] = frac;
        B->outCost[k] = calc_rd_cost(e, frac >> 15, B->outDist[k]);
      }
    }
    HM_SYNC();
    int slotBest = keep;
    for (int i = 0; i < nb; i++) {                                 // the reference's comparison, in list order: the best so far came earlier in the list
      const int slot = i + (keep >= 0 && i >= keep); const double v = B->outCost[slot];
      if (v < bestCost) { bestCost = v; slotBest = slot; best = c0 + i; }
    }
    keep = HM_UNI(slotBest); best = HM_UNI(best);
    c0 += nb;
#ifdef HM355_HOSTSIM
    batchesRun++;
#endif
  }
#ifdef HM355_HOSTSIM
  g_s16_stats.cand[numModes < 7 ? numModes : 7]++; g_s16_stats.batches[batchesRun < 3 ? batchesRun : 3]++;
#endif
  const int bestMode = HM_UNI(e->rdModeList[best]);
  e->s8Winner = keep | (best << 8);                                // simt_luma_winner_as_single_tu picks the winner's evaluation up from the overlays
  HM_SYNC();
  return bestMode;
}

// The closing pass of estIntraPredQT (:2566-2600) starts with the unsplit evaluation of the winner's transform block -- the very evaluation the
// candidates-in-lanes first pass (simt8_luma_first_pass, simt16_luma_first_pass) made for it, from the same snapshot.  Instead of repeating it
// (xIntraCodingTUBlock + xGetIntraBitsQT), the winner's results are put where the residual quadtree expects them: levels and reconstruction
// in the layer buffers of the block's size and in the picture, the estimator (e->cur) advanced past the block's syntax (the bins every candidate
// codes alike, then the contexts and the bit count of the winner's lane).  Must run right after the first pass (the overlays and the reference
// lines are still in place), with e->cur holding the CU's entry snapshot.  Distortion / bits / cbf in e->outDistY / e->outBits / e->outDist.
template <int L2> HM_DEV HM_NOINLINE void simt_luma_winner_as_single_tu(Shared *e, TU tv)
{
  HM_ENTRY(e); tv = hm_uni_struct(tv);
  const TU *t = &tv; WorkSpace *ws = e->ws;
  const Simt<L2> S(e);
  const int won = HM_UNI(e->s8Winner), best = won & 255, z = t->cuZ + t->relZ, ps = e->stride[0], bitDepth = e->bitDepth;
  const int mode = HM_UNI(e->rdModeList[won >> 8]), cbf = HM_UNI(sn_out_cbf(S)[best]);
  const SimtPar p = simt_params<L2>(e, 0);
  const int dcVal = ref_dc_val(e, 0, 1 << L2);
  Pel *rq = ws->qtRec[5 - L2] + t->y * 64 + t->x;
  Pel *recPic = e->fb.rec[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
  sn_dequant_inv1(S, p, best, cbf, ws->qtCoef[5 - L2] + z * 16, L2 == 3 ? intra_scan_type(mode) : SCAN_DIAG);
  sn_inv2_recon(S, bitDepth, cbf, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, 1 << L2, L2, x, y, dcVal, bitDepth); },
                [&](int x, int y, int rr) HM_LAMBDA_INL { rq[y * 64 + x] = (Pel)rr; recPic[y * ps + x] = (Pel)rr; });
  HM_SYNC();
  { // the estimator: the bins in front of the lane's own (same as the first pass counted), then the lane's contexts and bit count
    CabacR r; cabr_load(e, r, &e->cur);
    r.frac &= 32767;
    if (e->im) { code_skip_flag(e, &r, t->cuZ); enc_bin(e, &r, C_PRED_MODE, 1); }
    if (L2 == 3) enc_bin(e, &r, C_PART, 1);                          // 2Nx2N, coded at the smallest CU size only
    enc_bin(e, &r, C_SUBDIV + 5 - L2, 0);
    cabr_store(r, &e->cur);
  }
  simt_store_contexts(S, best, &e->cur, 1);
  e->cur.frac = (uint64_t)sn_out_frac(S)[best];
  e->outDistY = sn_out_dist(S)[best]; e->outBits = sn_out_frac(S)[best] >> 15; e->outDist = (uint32_t)cbf;
  HM_SYNC();
}
