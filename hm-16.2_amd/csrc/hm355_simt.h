// hm355 -- candidates in lanes: what the 4x4 batches (hm355_simt4.h), the 8x8 batches (hm355_simt8.h) and the 16x16 batches (hm355_simt16.h) share.
//
// One per-lane coefficient coder, parameterised by the block's log2 size L2 (2: one coefficient group, 3: four, 4: sixteen): the batch's
// tables (simt_setup), a context-coded bin on a job's private context copy (simt_bin), RDOQ (simt_rdoq =
// TComTrQuant::xRateDistOptQuant) and the bit count of the coefficients (simt_code_coeff = TEncSbac::codeCoeffNxN), in the
// reference's arithmetic and operation order -- the one-candidate-per-lane form of rdoq / code_coeff_nxn in hm355_core.h.
// Simt<L2> (defined by the size's header) holds the LDS overlays of a batch and hides where each size keeps its data:
//   tab(), ctx(c, k), lps()                  bit costs of the batch's start state, context copy c of job k, the LPS transitions
//   cs(sp, k), scan_pos(scanType, sp)        coefficient of job k at scan position sp; raster position of a scan position
//   put_dec / dec / mark_zeroed / zeroed     level of job k at decision time, and whether RDOQ zeroed its group afterwards
//   put_lev / lev                            final signed level of job k
//   cg_pos(scanType, cg)                     raster position of coefficient group cg
//   sig_inc(scanType, firstCtx, pattern, sp, chroma)   significance context increment
//   KEEPS_COST, keep_cost(), cost_at()       whether RDOQ stores the cost of each decided level (4x4) or prices it again (8x8, 16x16)
//   out_cbf / out_dist / out_frac / out_cost(k)   results of job k: coded block flag, distortion, Q15 bit count, RD cost
//   tile(stage), TS                          8x8, 16x16: the two stages of the transform tile under the lanes and its row stride
//   luma_scan(mode), ONE_BATCH               8x8, 16x16: scan type of a luma mode at this size; whether the longest candidate list fits one batch
// Then the small derivations the entry points have in common, the pricing of the five chroma modes of a CU (simt_pick_chroma_mode: 4x4 and
// 8x8 chroma blocks) and what 8x8 and 16x16 blocks share beyond the coder: the three sample passes (simt_residual_fwd, simt_dequant_inv1,
// simt_inv2_recon), the first pass over the candidates of a luma PU (simt_luma_first_pass) and the hand-over of its winner to the closing
// pass (simt_luma_winner_as_single_tu).  All are templates on L2, instantiated once the size's Simt<L2> is defined.  Included from
// hm355_core.h in front of the three.
#pragma once

// Context numbering inside a batch: X_* index the per-job context copies (Simt<L2>::A->ctx), T_* the bit costs of the batch's
// start state (A->tab, two entries per context: bin 0, bin 1).  Significance contexts by their increment, greater-than-1 contexts
// 4 * set + c1 with set = 0..3 for luma and 0..1 for chroma (whose sets are 4, 5 in the reference's numbering), greater-than-2 by
// set, the NLAST last-position contexts a block of this size uses per coordinate, the two coded-sub-block contexts (8x8), cbf,
// the prediction-mode bin, the transform-skip flag (4x4).  T_LASTX / T_LASTY hold the cost of each last-position group index.
template <int L2> struct SimtDim {
  enum { NC = 1 << (2 * L2), NCG = NC / 16, WCG = 1 << (L2 - 2), NSIG = L2 == 2 ? 9 : (L2 == 3 ? 21 : 27), NSET = NCG == 1 ? 1 : 4, NGRP = 2 * L2, NCGC = NCG == 1 ? 0 : 2,
         NLAST = L2 == 4 ? 4 : 3, LSH = L2 == 4 ? 1 : L2 - 2,   // last-position contexts per coordinate; group index -> context shift (a 16x16 block is luma only)
         X_SIG = 0, X_ONE = NSIG, X_ABS = X_ONE + 4 * NSET, X_LX = X_ABS + NSET, X_LY = X_LX + NLAST, X_CG = X_LY + NLAST, X_CBF = X_CG + NCGC,
         X_MODE = X_CBF + 1, X_TSKIP = X_MODE + 1, NCTX = X_TSKIP + (L2 == 2 ? 1 : 0),
         T_SIG = 0, T_ONE = 2 * NSIG, T_ABS = T_ONE + 8 * NSET, T_LASTX = T_ABS + 2 * NSET, T_LASTY = T_LASTX + NGRP, T_CG = T_LASTY + NGRP,
         T_CBF = T_CG + 2 * NCGC, T_N = T_CBF + 2 };
};
static_assert(SimtDim<2>::NCTX == 23 && SimtDim<2>::T_N == 38 && SimtDim<2>::X_LX == 14 && SimtDim<2>::X_LY == 17 && SimtDim<2>::X_CBF == 20 && SimtDim<2>::T_LASTX == 28 &&
              SimtDim<2>::T_LASTY == 32 && SimtDim<2>::T_CBF == 36 && SimtDim<2>::LSH == 0, "the 4x4 batch's numbering");
static_assert(SimtDim<3>::NCTX == 51 && SimtDim<3>::T_N == 100 && SimtDim<3>::X_ONE == 21 && SimtDim<3>::X_ABS == 37 && SimtDim<3>::X_LX == 41 && SimtDim<3>::X_LY == 44 &&
              SimtDim<3>::X_CG == 47 && SimtDim<3>::X_CBF == 49 && SimtDim<3>::T_ONE == 42 && SimtDim<3>::T_ABS == 74 && SimtDim<3>::T_LASTX == 82 && SimtDim<3>::T_LASTY == 88 &&
              SimtDim<3>::T_CG == 94 && SimtDim<3>::T_CBF == 98 && SimtDim<3>::LSH == 1 && SimtDim<3>::WCG == 2, "the 8x8 batch's numbering");
template <int L2> struct Simt;
template <int L2> struct SimtPrices {     // greater-than-1 / greater-than-2 prices of ic_rate in the batch's table
  const int32_t *tab;
  HM_FINL_M int one(int i) const { return tab[SimtDim<L2>::T_ONE + i]; }
  HM_FINL_M int abs2(int i) const { return tab[SimtDim<L2>::T_ABS + i]; }
};

struct SimtPar {                          // wave-uniform parameters of a batch
  int chroma, bitDepth, qBits, quantCoef, tshift; double errScale, lambda; int64_t rdFactor;
  int dqShift, dqScale, dqMin, dqMax;
};
template <int L2> HM_DEV inline SimtPar simt_params(const Shared *e, int chroma)
{
  SimtPar p;
  p.chroma = chroma; p.bitDepth = e->bitDepth; p.tshift = 15 - e->bitDepth - L2;
  p.qBits = 14 + e->fb.qpPer[chroma] + p.tshift; p.quantCoef = HM_QUANT_SCALES[e->fb.qpRem[chroma]];
  p.errScale = e->fb.errScale[chroma][L2 - 2]; p.lambda = chroma ? e->fb.lambdaC : e->fb.lambda; p.rdFactor = e->fb.rdFactor[chroma];
  p.dqShift = 6 - (p.tshift + e->fb.qpPer[chroma]); p.dqScale = HM_INV_QUANT_SCALES[e->fb.qpRem[chroma]];
  int tgt = 25 + p.dqShift; if (tgt > 16) tgt = 16;
  p.dqMin = -(1 << (tgt - 1)); p.dqMax = (1 << (tgt - 1)) - 1;
  return p;
}
HM_FINL int32_t simt_level_double(int sc, const SimtPar &p)
{
  const int64_t cap = 2147483647LL - (1LL << (p.qBits - 1));
  const int64_t tl = (int64_t)hm_abs(sc) * p.quantCoef;
  return (int32_t)(tl < cap ? tl : cap);
}
HM_FINL int simt_dequant(const SimtPar &p, int level)
{ // xDeQuant (flat), TComTrQuant.cpp:1276-1312
  const int c = hm_clip3(p.dqMin, p.dqMax, level);
  int v;
  if (p.dqShift > 0) v = (c * p.dqScale + (1 << (p.dqShift - 1))) >> p.dqShift;
  else v = (int)((unsigned)(c * p.dqScale) << (-p.dqShift));
  return hm_clip3(-32768, 32767, v);
}

// Cabac::s index of context copy j of a batch of component type `chroma`.  cbfCodeCtx: the cbf context the syntax codes with (index
// inside C_QT_CBF); modeCtx: the context of the prediction-mode bin the jobs code (C_INTRA_LUMA / C_CHROMA_PRED).
template <int L2> HM_FINL int simt_ctx_index(int j, int chroma, int cbfCodeCtx, int modeCtx)
{
  typedef SimtDim<L2> D;
  const int lastOff = chroma ? 15 : 3 * (L2 - 2);              // getLastSignificantContextParameters (last_ctx_params)
  if (j < D::X_ONE) return C_SIG + (chroma ? 28 : 0) + (chroma && j >= 16 ? 0 : j);
  if (j < D::X_ABS) return C_ONE + (chroma ? 16 + ((j - D::X_ONE) & 7) : j - D::X_ONE);
  if (j < D::X_LX) return C_ABS + (chroma ? 4 + ((j - D::X_ABS) & 1) : j - D::X_ABS);
  if (j < D::X_LY) return C_LASTX + lastOff + (j - D::X_LX);
  if (j < D::X_CG) return C_LASTY + lastOff + (j - D::X_LY);
  if (j < D::X_CBF) return C_SIG_CG + (chroma ? 2 : 0) + (j - D::X_CG);
  if (j == D::X_CBF) return C_QT_CBF + cbfCodeCtx;
  if (j == D::X_MODE) return modeCtx;
  return C_TSKIP + (chroma ? 1 : 0);
}
// Tables of a batch: bit costs of the start state `cb` for one component type (estBit, TEncSbac.cpp:1717-1956), the per-job
// context copies, the LPS transitions; the scans are the size's own (Simt<L2>::load_scans).  cbfCtx: index inside C_QT_CBF of
// the cbf RDOQ prices with.
template <int L2> HM_DEV inline void simt_setup(Shared *e, const Simt<L2> &S, const Cabac *cb, int jobs, int chroma, int cbfCtx, int cbfCodeCtx, int modeCtx)
{
  typedef SimtDim<L2> D;
  HM_PAR_FOR(i, D::T_N) {
    const int bin = i & 1;
    int v = 0;
    if (i < D::T_LASTX) {                 // the contexts in front of the last-position ones: same order in the table and in the copies
      const int j = i >> 1, none = chroma && ((j < D::X_ONE && j >= 16) || (j >= D::X_ONE && j < D::X_ABS && j - D::X_ONE >= 8) || (j >= D::X_ABS && j - D::X_ABS >= 2));
      if (!none) v = HM_LT()->ebits[cb->s[simt_ctx_index<L2>(j, chroma, 0, 0)] ^ bin];
    } else if (i < D::T_CG) { // last-position group index g: g ones on the contexts (c >> LSH) of the block's NLAST, then a zero unless g is the maximum; g > 3 adds bypass bits (xGetRateLast :2815)
      const int g = (i - D::T_LASTX) % D::NGRP, x0 = i < D::T_LASTY ? D::X_LX : D::X_LY;
      for (int c = 0; c < g; c++) v += HM_LT()->ebits[cb->s[simt_ctx_index<L2>(x0 + (c >> D::LSH), chroma, 0, 0)] ^ 1];
      if (g < D::NGRP - 1) v += HM_LT()->ebits[cb->s[simt_ctx_index<L2>(x0 + (g >> D::LSH), chroma, 0, 0)] ^ 0];
      if (g > 3) v += 32768 * ((g - 2) >> 1);
    } else if (i < D::T_CBF) v = HM_LT()->ebits[cb->s[simt_ctx_index<L2>(D::X_CG + ((i - D::T_CG) >> 1), chroma, 0, 0)] ^ bin];
    else v = HM_LT()->ebits[cb->s[C_QT_CBF + cbfCtx] ^ bin];
    S.tab()[i] = v;
  }
  HM_PAR_FOR(i, 128) S.lps()[i] = HM_NEXT_LPS[i];
  HM_PAR_FOR(i, D::NCTX * S.JOBS) {
    const int j = i / S.JOBS, k = i - j * S.JOBS;
    if (k < jobs) S.ctx(j, k) = cb->s[simt_ctx_index<L2>(j, chroma, cbfCodeCtx, modeCtx)];
  }
  S.load_scans(e);
  HM_SYNC();
}
// the estimator after job k of a luma batch: the contexts the lane advanced
template <int L2> HM_FINL void simt_store_contexts(const Simt<L2> &S, int k, Cabac *cb, int cbfCodeCtx)
{
  HM_PAR_FOR(j, SimtDim<L2>::NCTX) cb->s[simt_ctx_index<L2>(j, 0, cbfCodeCtx, C_INTRA_LUMA)] = S.ctx(j, k);
}
// the estimator after job k of a chroma-mode batch (simt4_chroma_cu, simt8_chroma_cu16: cbf at the CU's root TU, the chroma prediction mode): the
// contexts the lane advanced and its Q15 count.  The copies a chroma block has no context for (simt_setup's `none`) alias others and are left out.
template <int L2> HM_FINL void simt_store_chroma_mode(const Simt<L2> &S, int k, Cabac *cb, uint32_t frac)
{
  typedef SimtDim<L2> D;
  HM_PAR_FOR(j, D::NCTX) {
    const int none = (j < D::X_ONE && j >= 16) || (j >= D::X_ONE && j < D::X_ABS && j - D::X_ONE >= 8) || (j >= D::X_ABS && j < D::X_LX && j - D::X_ABS >= 2);
    if (!none) cb->s[simt_ctx_index<L2>(j, 1, 5, C_CHROMA_PRED)] = S.ctx(j, k);
  }
  cb->frac = (uint64_t)frac;
}

// one context-coded bin on job k's private context copy; frac counts Q15 bits
template <int L2> HM_DEV inline void simt_bin(const Shared *e, const Simt<L2> &S, int k, uint32_t *frac, int c, int bin)
{
  const int st = S.ctx(c, k);
  *frac += (uint32_t)HM_LT()->ebits[st ^ bin];
  S.ctx(c, k) = (uint8_t)(bin == (st & 1) ? (st < 124 ? st + 2 : st) : S.lps()[st]);
}
// calcPatternSigCtx / getSigCoeffGroupCtxInc: the coded flags of the groups right of and below the one at cgBlkPos (WCG groups per row)
template <int L2> HM_FINL int simt_cg_pattern(int cgBlkPos, int cgMask)
{
  const int W = SimtDim<L2>::WCG, cgx = cgBlkPos & (W - 1), cgy = cgBlkPos >> (L2 - 2);
  const int sigRight = cgx < W - 1 ? ((cgMask >> (cgBlkPos + 1)) & 1) : 0, sigLower = cgy < W - 1 ? ((cgMask >> (cgBlkPos + W)) & 1) : 0;
  return sigRight + (sigLower << 1);
}
// raster position -> (x, y) of the last-position syntax (swapped for the vertical scan)
template <int L2> HM_FINL void simt_last_xy(int blkPos, int scanType, int *px, int *py)
{
  const int y = blkPos >> L2, x = blkPos & ((1 << L2) - 1);
  *px = scanType == SCAN_VER ? y : x; *py = scanType == SCAN_VER ? x : y;
}

// RDOQ of job k's block (TComTrQuant::xRateDistOptQuant, TComTrQuant.cpp:1974-2511): coefficients in S.cs(., k) (scan order); leaves the
// signed levels in S.lev(., k) (level at decision time in S.dec(., k)) and returns the sum of their magnitudes.
template <int L2> HM_DEV inline int simt_rdoq(const Simt<L2> &S, const SimtPar &p, int k, int scanType)
{
  typedef SimtDim<L2> D;
  const int32_t *tab = S.tab(); const SimtPrices<L2> prices = { tab };
  const int qBits = p.qBits, half = 1 << (qBits - 1);
  const double lambda = p.lambda, errScale = p.errScale;
  const int firstCtx = first_sig_ctx(1 << L2, scanType, p.chroma), lumaSets = p.chroma ? 0 : 2;      // luma: coefficient groups behind the first use context sets 2, 3
  double blockUncoded = 0, baseCost = 0;
  int last = -1, cgLast = -1, ctxSet = 0;
  int cgMask = 0; uint32_t cgSets = 0;                            // group flags (bit = raster position of the group); context set each group started with (two bits per group)
  LevelChain ch;
  for (int cg = D::NCG - 1; cg >= 0; cg--) {
    const int cgBlkPos = S.cg_pos(scanType, cg), cgBit = 1 << cgBlkPos, pattern = simt_cg_pattern<L2>(cgBlkPos, cgMask);
    double sigCost = 0, sigCost0 = 0, codedLevelAndDist = 0, uncodedDist = 0; int nnzBeforePos0 = 0;
    cgSets |= (uint32_t)ctxSet << (2 * cg);
    for (int q = 15; q >= 0; q--) {
      const int sp = cg * 16 + q;
      const int32_t lvlD = simt_level_double(S.cs(sp, k), p);
      uint32_t mx = (uint32_t)((lvlD + half) >> qBits); if (mx > 32767u) mx = 32767u;
      const double err = (double)lvlD, c0 = err * err * errScale;
      blockUncoded += c0;
      if (mx > 0 && last < 0) { last = sp; cgLast = cg; ctxSet = cg > 0 ? lumaSets : 0; cgSets = (uint32_t)ctxSet << (2 * cg); }
      uint32_t level = 0; double cSig = 0, cCoeff = c0;
      if (last >= 0) {
        const int isLast = (sp == last);
        const int si = isLast ? 0 : S.sig_inc(scanType, firstCtx, pattern, sp, p.chroma);
        if (!isLast && mx < 3) { cSig = lambda * (double)tab[D::T_SIG + si * 2]; cCoeff = c0 + cSig; }      // xGetCodedLevel :2660
        else cCoeff = HM_MAX_DOUBLE;
        if (mx > 0) {
          double currCostSig = 0;
          if (!isLast) currCostSig = lambda * (double)tab[D::T_SIG + si * 2 + 1];
          const uint32_t minAbs = mx > 1 ? mx - 1 : 1;
          for (int al = (int)mx; al >= (int)minAbs; al--) {
            const double de = (double)(lvlD - (int32_t)((uint32_t)al << qBits));
            const double dist = de * de * errScale;
            const double rc = lambda * (double)ic_rate(prices, (uint32_t)al, 4 * ctxSet + ch.c1, ctxSet, ch);
            double cc = dist + rc;
            cc += currCostSig;
            if (cc < cCoeff) { level = (uint32_t)al; cCoeff = cc; cSig = currCostSig; }
          }
        }
        S.keep_cost(sp, k, cCoeff);
        baseCost += cCoeff;
        ch.step(level);
        if (q == 0 && cg > 0) { ctxSet = ((cg - 1) > 0 ? lumaSets : 0) + (ch.c1 == 0 ? 1 : 0); ch = LevelChain(); }
      } else baseCost += c0;
      sigCost += cSig;
      if (q == 0) sigCost0 = cSig;
      if (level) {
        cgMask |= cgBit;
        codedLevelAndDist += cCoeff - cSig;
        uncodedDist += c0;
        if (q != 0) nnzBeforePos0++;
      }
      S.put_dec(sp, k, level);
    }
    if (cgLast >= 0) {
      if (cg) {
        const int cgCtx = (pattern != 0) * 2;                                              // getSigCoeffGroupCtxInc :2872
        if (!(cgMask & cgBit)) {
          const double r0 = lambda * (double)tab[D::T_CG + cgCtx];
          baseCost += r0 - sigCost;
        } else if (cg < cgLast) {
          if (nnzBeforePos0 == 0) { baseCost -= sigCost0; sigCost -= sigCost0; }
          double costZeroCG = baseCost;
          const double r0 = lambda * (double)tab[D::T_CG + cgCtx], r1 = lambda * (double)tab[D::T_CG + cgCtx + 1];
          baseCost += r1;
          costZeroCG += r0;
          costZeroCG += uncodedDist; costZeroCG -= codedLevelAndDist; costZeroCG -= sigCost;
          if (costZeroCG < baseCost) {
            cgMask &= ~cgBit; baseCost = costZeroCG;
            for (int q = 15; q >= 0; q--) S.mark_zeroed(cg * 16 + q, k);          // the decision-time level stays for the walks below
          }
        }
      } else cgMask |= cgBit;
    }
  }
  if (last < 0) return 0;
  double bestCost = blockUncoded + lambda * (double)tab[D::T_CBF];            // TComTrQuant.cpp:2310-2316
  baseCost += lambda * (double)tab[D::T_CBF + 1];
  int bestLastP1 = 0, found = 0;
  for (int cg = cgLast; cg >= 0 && !found; cg--) {
    // the cost the decision loop added for the group's coded-sub-block flag, priced again: none for the last group, else the flag the group
    // ended up with on the context its right and lower neighbours gave it (both were settled before the group itself was decided).  The
    // group of the last position adds none because it always stays coded: the level decided at the last position is at least 1 (its zero
    // hypothesis costs HM_MAX_DOUBLE), so that group never takes the uncoded branch that would have added the price of a 0 flag.
    const int cgBlkPos = S.cg_pos(scanType, cg), coded = (cgMask >> cgBlkPos) & 1, pattern = simt_cg_pattern<L2>(cgBlkPos, cgMask);
    if (cg && cg < cgLast) baseCost -= lambda * (double)tab[D::T_CG + (pattern != 0) * 2 + coded];
    if (!coded) continue;
    // the decision chain's state inside this group, walked again where the levels it decided are priced again
    const int wSet = (int)((cgSets >> (2 * cg)) & 3); LevelChain walk;
    for (int q = (cg == cgLast ? (last & 15) : 15); q >= 0; q--) {
      const int sp = cg * 16 + q, lev = S.dec(sp, k);
      const int si = sp == last ? 0 : S.sig_inc(scanType, firstCtx, pattern, sp, p.chroma);
      if (lev) {
        int px, py; simt_last_xy<L2>(S.scan_pos(scanType, sp), scanType, &px, &py);
        const double costLast = lambda * (double)(tab[D::T_LASTX + hm_group_idx(px)] + tab[D::T_LASTY + hm_group_idx(py)]);
        const double cSig = (sp == last) ? 0.0 : lambda * (double)tab[D::T_SIG + si * 2 + 1];
        const double t1 = baseCost + costLast;
        const double totalCost = t1 - cSig;
        if (totalCost < bestCost) { bestLastP1 = sp + 1; bestCost = totalCost; }
        if (lev > 1) { found = 1; break; }
        const int32_t lvlD = simt_level_double(S.cs(sp, k), p);
        const double err = (double)lvlD;
        double cc;
        if (S.KEEPS_COST) cc = S.cost_at(sp, k);
        else {
          const double de = (double)(lvlD - (int32_t)((uint32_t)lev << qBits));
          const double dist = de * de * errScale;
          const double rc = lambda * (double)ic_rate(prices, (uint32_t)lev, 4 * wSet + walk.c1, wSet, walk);
          cc = dist + rc;
          cc += cSig;
          walk.step((uint32_t)lev);
        }
        baseCost -= cc; baseCost += err * err * errScale;
      } else baseCost -= lambda * (double)tab[D::T_SIG + si * 2];
    }
  }
  // levels with signs: zeroed groups and everything behind the chosen last position become 0
  int absSum = 0;
  for (int sp = 0; sp < D::NC; sp++) {
    const int lv = (sp < bestLastP1 && !S.zeroed(sp, k)) ? S.dec(sp, k) : 0;
    absSum += lv;
    S.put_lev(sp, k, S.cs(sp, k) < 0 ? -lv : lv);
  }
  // sign bit hiding, TComTrQuant.cpp:2380-2510
  if (absSum >= 2) {
    int lastCG = -1;
    for (int subSet = D::NCG - 1; subSet >= 0; subSet--) {
      const int subPos = subSet << 4;
      int lastNZ = -1, firstNZ = 16, parity = 0;
      for (int q = 0; q < 16; q++) { const int lv = S.lev(subPos + q, k); if (lv) { lastNZ = q; if (firstNZ == 16) firstNZ = q; } parity ^= lv & 1; }
      if (lastNZ >= 0 && lastCG == -1) lastCG = 1;
      if (lastNZ - firstNZ >= 4) {
        const uint32_t signbit = S.lev(subPos + firstNZ, k) > 0 ? 0 : 1;
        if (signbit != (uint32_t)parity) {
          const int64_t I64MAX = 0x7fffffffffffffffLL;
          int64_t minCostInc = I64MAX, curCost = I64MAX; int minK = -1, finalChange = 0, curChange = 0;
          const int wSet = (int)((cgSets >> (2 * subSet)) & 3); LevelChain walk;   // the decision chain's state, walked again
          const int top = (subPos + 15 <= last) ? 15 : (last - subPos), kStart = (lastCG == 1 ? lastNZ : 15);
          const int pattern = simt_cg_pattern<L2>(S.cg_pos(scanType, subSet), cgMask);
          for (int q = top; q >= 0; --q) {
            const uint32_t dec = (uint32_t)S.dec(subPos + q, k); const int dv = S.lev(subPos + q, k);
            const int ctxOne = 4 * wSet + walk.c1; const LevelChain at = walk;
            walk.step(dec);
            if (q > kStart) continue;
            const int sc = S.cs(subPos + q, k);
            const int32_t lvlD = simt_level_double(sc, p);
            const int32_t deltaU = (int32_t)((lvlD - (int32_t)(dec << qBits)) >> (qBits - 8));
            const int si = (subPos + q == last) ? 0 : S.sig_inc(scanType, firstCtx, pattern, subPos + q, p.chroma);
            const int sigRateDelta = (subPos + q == last) ? 0 : tab[D::T_SIG + si * 2 + 1] - tab[D::T_SIG + si * 2];
            int rateIncUp, rateIncDown = 0;
            if (dec > 0) {
              const int rateNow = ic_rate(prices, dec, ctxOne, wSet, at);
              rateIncUp = ic_rate(prices, dec + 1, ctxOne, wSet, at) - rateNow;
              rateIncDown = ic_rate(prices, dec - 1, ctxOne, wSet, at) - rateNow;
            } else rateIncUp = prices.one(ctxOne * 2);
            if (dv != 0) {
              const int64_t costUp = p.rdFactor * (-deltaU) + rateIncUp;
              int64_t costDown = p.rdFactor * (deltaU) + rateIncDown - ((hm_abs(dv) == 1) ? sigRateDelta : 0);
              if (lastCG == 1 && lastNZ == q && hm_abs(dv) == 1) costDown -= (4 << 15);
              if (costUp < costDown) { curCost = costUp; curChange = 1; }
              else { curChange = -1; if (q == firstNZ && hm_abs(dv) == 1) curCost = I64MAX; else curCost = costDown; }
            } else {
              curCost = p.rdFactor * (-(hm_abs(deltaU))) + (1 << 15) + rateIncUp + sigRateDelta;
              curChange = 1;
              if (q < firstNZ) { const uint32_t thissign = sc < 0 ? 1u : 0u; if (thissign != signbit) curCost = I64MAX; }
            }
            if (curCost < minCostInc) { minCostInc = curCost; finalChange = curChange; minK = q; }
          }
          if (minK >= 0) {
            int mv = S.lev(subPos + minK, k);
            if (mv == 32767 || mv == -32768) finalChange = -1;
            mv = (S.cs(subPos + minK, k) < 0) ? mv - finalChange : mv + finalChange;
            S.put_lev(subPos + minK, k, mv);
          }
        }
      }
      if (lastCG == 1) lastCG = 0;
    }
  }
  return absSum;
}

// TEncSbac::codeCoeffNxN, TEncSbac.cpp:1172-1525, of a block on job k's private contexts (bits only): the levels are
// S.lev(., src) (job `src` evaluated the block; k codes it).  The transform-skip flag of a 4x4 block is the caller's.
template <int L2> HM_DEV inline void simt_code_coeff(const Shared *e, const Simt<L2> &S, int k, int src, int chroma, int scanType, uint32_t *frac)
{
  typedef SimtDim<L2> D;
  int last = -1, cgMask = 0;
  for (int sp = 0; sp < D::NC; sp++)
    if (S.lev(sp, src) != 0) { last = sp; cgMask |= 1 << S.cg_pos(scanType, sp >> 4); }
  { // codeLastSignificantXY :1106: the group index of each coordinate on the block's three contexts, then its bypass suffix
    int px, py; simt_last_xy<L2>(S.scan_pos(scanType, last), scanType, &px, &py);
    const int gx = hm_group_idx(px), gy = hm_group_idx(py);
    int q;
    for (q = 0; q < gx; q++) simt_bin(e, S, k, frac, D::X_LX + (q >> D::LSH), 1);
    if (gx < D::NGRP - 1) simt_bin(e, S, k, frac, D::X_LX + (q >> D::LSH), 0);
    for (q = 0; q < gy; q++) simt_bin(e, S, k, frac, D::X_LY + (q >> D::LSH), 1);
    if (gy < D::NGRP - 1) simt_bin(e, S, k, frac, D::X_LY + (q >> D::LSH), 0);
    if (gx > 3) *frac += 32768u * (uint32_t)((gx - 2) >> 1);
    if (gy > 3) *frac += 32768u * (uint32_t)((gy - 2) >> 1);
  }
  const int firstCtx = first_sig_ctx(1 << L2, scanType, chroma), lastSet = last >> 4;
  int c1 = 1;
  for (int subSet = lastSet; subSet >= 0; subSet--) {
    const int subPos = subSet << 4, isLastSet = subSet == lastSet;
    const int cgBlkPos = S.cg_pos(scanType, subSet), pattern = simt_cg_pattern<L2>(cgBlkPos, cgMask);
    if (isLastSet || subSet == 0) cgMask |= 1 << cgBlkPos;            // coded-sub-block flag: implied for the last group and the first
    else simt_bin(e, S, k, frac, D::X_CG + (pattern != 0), (cgMask >> cgBlkPos) & 1);
    if (!((cgMask >> cgBlkPos) & 1)) continue;
    const int top = isLastSet ? (last & 15) : 15;
    int numNonZero = isLastSet ? 1 : 0, firstNZ = isLastSet ? top : 16, lastNZ = isLastSet ? top : -1;
    for (int q = isLastSet ? top - 1 : 15; q >= 0; q--) {           // significance flags; the last coefficient itself is implied
      const int sig = S.lev(subPos + q, src) != 0;
      if (q > 0 || subSet == 0 || numNonZero) simt_bin(e, S, k, frac, D::X_SIG + S.sig_inc(scanType, firstCtx, pattern, subPos + q, chroma), sig);
      if (sig) { numNonZero++; firstNZ = q; if (lastNZ < 0) lastNZ = q; }
    }
    if (numNonZero > 0) {
      const int signHidden = (lastNZ - firstNZ >= 4);
      const int ctxSet = ((subSet > 0 && !chroma) ? 2 : 0) + (c1 == 0 ? 1 : 0);
      c1 = 1;
      int firstC2 = -1, escape = 0, idx = 0;
      for (int q = lastNZ; q >= 0 && idx < 8; q--) {
        const int a = hm_abs(S.lev(subPos + q, src));
        if (!a) continue;
        const int sym = a > 1;
        simt_bin(e, S, k, frac, D::X_ONE + 4 * ctxSet + c1, sym);
        if (sym) { c1 = 0; if (firstC2 == -1) firstC2 = q; else escape = 1; }
        else if (c1 < 3 && c1 > 0) c1++;
        idx++;
      }
      if (c1 == 0 && firstC2 != -1) { const int sym = hm_abs(S.lev(subPos + firstC2, src)) > 2; simt_bin(e, S, k, frac, D::X_ABS + ctxSet, sym); if (sym) escape = 1; }
      escape = escape || (numNonZero > 8);
      *frac += 32768u * (uint32_t)(signHidden ? numNonZero - 1 : numNonZero);
      if (escape) {
        int firstCoeff2 = 1; uint32_t goRice = 0; idx = 0;
        for (int q = lastNZ; q >= 0; q--) {
          const int a = hm_abs(S.lev(subPos + q, src));
          if (!a) continue;
          const int baseLevel = (idx < 8) ? (2 + firstCoeff2) : 1;
          if (a >= baseLevel) {
            *frac += 32768u * coef_remain_len((uint32_t)(a - baseLevel), goRice);
            if ((uint32_t)a > (3u << goRice)) goRice = goRice + 1 < 4 ? goRice + 1 : 4;
          }
          if (a >= 2) firstCoeff2 = 0;
          idx++;
        }
      }
    }
  }
}

// ---- small derivations of the entry points
// bits of a luma candidate's prediction mode (codeIntraDirLumaAng :636): the most-probable-mode flag on job k's contexts, then the index or the remainder
template <int L2> HM_FINL void simt_luma_mode_bits(const Shared *e, const Simt<L2> &S, int k, uint32_t *frac, int mode)
{
  int predIdx = -1;
  for (int i = 0; i < 3; i++) if (mode == e->mpmPreds[i]) predIdx = i;
  simt_bin(e, S, k, frac, SimtDim<L2>::X_MODE, predIdx != -1);
  *frac += 32768u * (uint32_t)(predIdx == -1 ? 5 : (predIdx ? 2 : 1));
}
// the unfiltered reference lines of the two n x n chroma blocks at (px, py): Cr into slot 1, Cb into slot 0 (chroma never uses the smoothed lines)
HM_FINL void simt_chroma_ref_lines(Shared *e, int px, int py, int n, int x4, int y4)
{
  init_adi_pattern(e, 2, px, py, n, x4, y4, n >> 1, 0);
  HM_PAR_FOR(i, 2 * n + 1) { e->u.ref.refTop[1][i] = e->u.ref.refTop[0][i]; e->u.ref.refLeft[1][i] = e->u.ref.refLeft[0][i]; }
  HM_SYNC();
  init_adi_pattern(e, 1, px, py, n, x4, y4, n >> 1, 0);
}
// getAllowedChromaDir, TComDataCU.cpp:1486: planar, vertical, horizontal, DC with the one equal to the luma mode replaced by 34, then the luma mode itself
HM_FINL void allowed_chroma_dirs(int lumaDir, int *list)
{
  list[0] = PLANAR_IDX; list[1] = VER_IDX; list[2] = HOR_IDX; list[3] = DC_IDX; list[4] = DM_CHROMA_IDX;
  for (int i = 0; i < 4; i++) if (lumaDir == list[i]) { list[i] = 34; break; }
}
HM_FINL int chroma_mode_at(const int *list, int mi)              // list[mi] for a per-lane mi, with the list staying in registers
{ return mi == 0 ? list[0] : (mi == 1 ? list[1] : (mi == 2 ? list[2] : (mi == 3 ? list[3] : list[4]))); }

// ---- the five chroma modes of a CU, jobs 2 * modeIndex + component - 1 evaluated (out_cbf, out_dist): lane 2 * modeIndex counts the mode's
// bits on its own context copy -- chroma prediction mode (codeIntraDirChroma :692), both cbfs at the CU's root TU (xEncSubdivCbfQT :856), Cb then
// Cr coefficients (xGetIntraBitsQT :1038) -- and its cost; then the reference's comparison in list order, strict "<".  code(k, src, &frac): the
// coefficient bits of job src's block on lane k's contexts (the size's coder with its scan).  Returns the winning mode's index; its Q15 count
// stays in out_frac(2 * index).
template <int L2, class Code> HM_FINL int simt_pick_chroma_mode(const Shared *e, const Simt<L2> &S, uint32_t baseFrac, const int *modeList, Code code)
{
  HM_WAVE_FOR(k) {
    if (k < 10 && !(k & 1)) {
      const int dirC = chroma_mode_at(modeList, k >> 1);
      uint32_t frac = baseFrac;
      simt_bin(e, S, k, &frac, SimtDim<L2>::X_MODE, dirC != DM_CHROMA_IDX);
      if (dirC != DM_CHROMA_IDX) frac += 2u * 32768u;
      const int cbfU = S.out_cbf(k), cbfV = S.out_cbf(k + 1);
      simt_bin(e, S, k, &frac, SimtDim<L2>::X_CBF, cbfU);
      simt_bin(e, S, k, &frac, SimtDim<L2>::X_CBF, cbfV);
      if (cbfU) code(k, k, &frac);
      if (cbfV) code(k, k + 1, &frac);
      S.out_frac(k) = frac;
      S.out_cost(k) = calc_rd_cost(e, frac >> 15, S.out_dist(k) + S.out_dist(k + 1));
    }
  }
  HM_SYNC();
  double bestCost = HM_MAX_DOUBLE; int best = 0;
  for (int mi = 0; mi < 5; mi++) { const double v = S.out_cost(2 * mi); if (v < bestCost) { bestCost = v; best = mi; } }
  return HM_UNI(best);
}

// ------------------------------------------------------------------------------------------------
// Blocks of 8x8 and 16x16 samples (L2 = 3, 4): the wavefront alternates between two shapes of parallelism,
//   * sample work (prediction, residual, the transforms, de-quantisation, reconstruction, SSE) one job after the other with the 64 lanes
//     on the block's samples -- the three passes below, over the batch's transform tile S.tile(stage) with rows of Simt<L2>::TS entries,
//   * the serial chains (simt_rdoq, simt_code_coeff) for all jobs at once, one job per lane.
// pred(x, y): the predicted sample.  The transforms are the plain matrix products (rows (32 >> L2) * k of the 32-point matrix): sums of exact
// integer products, so they give the partial butterflies' integers.
// ------------------------------------------------------------------------------------------------
// residual + forward transform (xTrMxN :836); coefficients to A->cs[.][job] in the scan order `scanType`
template <int L2, class Pred> HM_FINL void simt_residual_fwd(const Simt<L2> &S, const Pel *org, int ps, int bitDepth, int scanType, int job, Pred pred)
{
  enum { N = 1 << L2, T = Simt<L2>::TS, ROW = (32 >> L2) * HM_TSTRIDE };
  int32_t *t0 = S.tile(0), *t1 = S.tile(1);
  const int s1 = L2 + bitDepth - 9, a1 = 1 << (s1 - 1), s2 = L2 + 6, a2 = 1 << (s2 - 1);
  HM_PAR_FOR(l, N * N) { const int y = l >> L2, x = l & (N - 1); t0[y * T + x] = org[y * ps + x] - pred(x, y); }
  HM_SYNC();
  HM_PAR_FOR(l, N * N) { // first stage
    const int j = l >> L2, kk = l & (N - 1); int32_t acc = 0;
    for (int i = 0; i < N; i++) acc += HM_LT()->tmat[kk * ROW + i] * t0[j * T + i];
    t1[kk * T + j] = (acc + a1) >> s1;
  }
  HM_SYNC();
  HM_PAR_FOR(l, N * N) { // second stage, one lane per scan position
    const int blkPos = S.scan_pos(scanType, l), kk = blkPos >> L2, j = blkPos & (N - 1); int32_t acc = 0;
    for (int i = 0; i < N; i++) acc += HM_LT()->tmat[kk * ROW + i] * t1[j * T + i];
    S.A->cs[l][job] = (int16_t)((acc + a2) >> s2);
  }
  HM_SYNC();
}
// de-quantisation of job's levels into raster order + first inverse stage (xITrMxN :894); coef: where to store the levels as well, or null
template <int L2> HM_FINL void simt_dequant_inv1(const Simt<L2> &S, const SimtPar &p, int scanType, int job, int cbf, TCoeff *coef)
{
  enum { N = 1 << L2, T = Simt<L2>::TS, ROW = (32 >> L2) * HM_TSTRIDE };
  int32_t *t0 = S.tile(0), *t1 = S.tile(1);
  if (cbf) {
    HM_PAR_FOR(l, N * N) {
      const int lv = S.lev(l, job), blk = S.scan_pos(scanType, l);
      if (coef) coef[blk] = lv;
      t0[(blk >> L2) * T + (blk & (N - 1))] = simt_dequant(p, lv);
    }
    HM_SYNC();
    HM_PAR_FOR(l, N * N) {
      const int j = l >> L2, i = l & (N - 1); int32_t acc = 0;
      for (int kk = 0; kk < N; kk++) acc += HM_LT()->tmat[kk * ROW + i] * t0[kk * T + j];
      t1[j * T + i] = hm_clip3(-32768, 32767, (acc + 64) >> 7);
    }
    HM_SYNC();
  } else if (coef) { HM_PAR_FOR(l, N * N) coef[l] = 0; }
}
// second inverse stage + prediction + clip: out(x, y, reconstructed sample)
template <int L2, class Pred, class Out> HM_FINL void simt_inv2_recon(const Simt<L2> &S, int bitDepth, int cbf, Pred pred, Out out)
{
  enum { N = 1 << L2, T = Simt<L2>::TS, ROW = (32 >> L2) * HM_TSTRIDE };
  const int32_t *t1 = S.tile(1);
  const int maxv = (1 << bitDepth) - 1, is2 = 20 - bitDepth;
  HM_PAR_FOR(l, N * N) {
    const int j = l >> L2, i = l & (N - 1); int resi = 0;
    if (cbf) {
      int32_t acc = 0;
      for (int kk = 0; kk < N; kk++) acc += HM_LT()->tmat[kk * ROW + i] * t1[kk * T + j];
      resi = hm_clip3(-32768, 32767, (acc + (1 << (is2 - 1))) >> is2);
    }
    out(i, j, hm_clip3(0, maxv, pred(i, j) + resi));
  }
}

#ifdef HM355_HOSTSIM
// host twin only: how many candidates the first passes of each size had and how many batches they took (printed at exit when HM355_S16_STATS is set)
#include <stdio.h>
struct SimtFirstPassStats {
  unsigned long cand[2][12], batches[2][4];
  ~SimtFirstPassStats()
  {
    if (!getenv("HM355_S16_STATS")) return;
    for (int s = 1; s >= 0; s--) {
      fprintf(stderr, "s%d candidates", 8 << s); for (int i = 0; i < (s ? 8 : 12); i++) fprintf(stderr, " %lu", cand[s][i]);
      fprintf(stderr, "\ns%d batches", 8 << s); for (int i = 0; i < 4; i++) fprintf(stderr, " %lu", batches[s][i]);
      fprintf(stderr, "\n");
    }
  }
};
static SimtFirstPassStats g_first_pass_stats;
#endif

// the bins every candidate of an unsplit 2Nx2N luma PU codes alike, in front of its own (xEncIntraHeader :965, xEncSubdivCbfQT :856)
template <int L2> HM_FINL void simt_luma_common_bins(Shared *e, CabacR *r, int cuZ)
{
  r->frac &= 32767;
  if (e->im) { code_skip_flag(e, r, cuZ); enc_bin(e, r, C_PRED_MODE, 1); }
  if (L2 == 3) enc_bin(e, r, C_PART, 1);                           // 2Nx2N, coded at the smallest CU size only
  enc_bin(e, r, C_SUBDIV + 5 - L2, 0);                             // transform_split of the root TU: not split in this pass
}

// ------------------------------------------------------------------------------------------------
// The first pass of estIntraPredQT (:2473-2490) over the RD candidates e->rdModeList[0..numModes) of the 8x8 or 16x16 luma PU `tv` (a 2Nx2N CU
// of depth 3 or 2).  Every candidate is the same evaluation of one unsplit transform block from the same CABAC snapshot (xRecurIntraCodingQT
// with bCheckFirst: no split), and only its cost is kept -- the closing pass picks the winner's evaluation up (simt_luma_winner_as_single_tu)
// and goes on with the full residual quadtree.  e->cur holds the CU's entry snapshot, e->u.ref the PU's reference samples (both the plain and
// the smoothed lines), e->mpmPreds its most probable modes.
// The candidates run in batches of Simt<L2>::JOBS, in list order: member i of a batch (candidate c0 + i) takes slot i, stepping over the slot
// of the best candidate so far, which stays where it is (its levels, contexts and results are what the closing pass picks up).  Where the
// largest list fits one batch (Simt<L2>::ONE_BATCH: 8x8) no slot is ever kept, which the compiler knows.
// Returns the winning mode: the candidate of least cost, the first one on a tie (estIntraPredQT :2520-2560); e->s8Winner: its slot and its
// place in the list.
// ------------------------------------------------------------------------------------------------
template <int L2> HM_DEV HM_NOINLINE int simt_luma_first_pass(Shared *e, TU tv, int numModes)
{
  enum { N = 1 << L2, JOBS = Simt<L2>::JOBS, ONE = Simt<L2>::ONE_BATCH };
  HM_ENTRY(e); numModes = HM_UNI(numModes); tv = hm_uni_struct(tv);
  const TU *t = &tv;
  const int ps = e->stride[0], bitDepth = e->bitDepth;
  const Simt<L2> S(e);
  uint32_t commonFrac;
  {
    CabacR r; cabr_load(e, r, &e->cur);
    simt_luma_common_bins<L2>(e, &r, t->cuZ);
    commonFrac = (uint32_t)r.frac;
  }
  simt_setup(e, S, &e->cur, ONE || numModes < JOBS ? numModes : JOBS, 0, 1, 1, C_INTRA_LUMA);       // luma cbf at the CU's root TU: context 1
  const SimtPar p = simt_params<L2>(e, 0);
  const Pel *org = e->fb.org[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
  const int dcVal = ref_dc_val(e, 0, N), shiftSse = (bitDepth - 8) << 1;
  double bestCost = HM_MAX_DOUBLE; int kept = -1, best = 0;        // kept: the slot of the best candidate so far (none before the first batch)
#ifdef HM355_HOSTSIM
  int batchesRun = 0;
#endif
  for (int c0 = 0; c0 < numModes;) {
    const int keep = ONE ? -1 : kept;
    const int room = keep < 0 ? JOBS : JOBS - 1, nb = ONE || numModes - c0 < room ? numModes - c0 : room;
    if (keep >= 0) {                                               // fresh context copies for the slots that are used again
      HM_PAR_FOR(i, SimtDim<L2>::NCTX * JOBS) {
        const int j = i / JOBS, k = i - j * JOBS;
        if (k != keep) S.ctx(j, k) = e->cur.s[simt_ctx_index<L2>(j, 0, 1, C_INTRA_LUMA)];
      }
      HM_SYNC();
    }
    // ---- residual + forward transform of every candidate, lanes on the samples; coefficients to A->cs in the candidate's scan order
    for (int i = 0; i < nb; i++) {
      const int slot = i + (keep >= 0 && i >= keep), mode = HM_UNI(e->rdModeList[c0 + i]);
      simt_residual_fwd(S, org, ps, bitDepth, S.luma_scan(mode), slot, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, N, L2, x, y, dcVal, bitDepth); });
    }
    // ---- level decision of every candidate, one per lane
    HM_WAVE_FOR(k) {
      const int i = (keep >= 0 && k > keep) ? k - 1 : k;
      if ((ONE || k < JOBS) && k != keep && i < nb) S.out_cbf(k) = (uint8_t)(simt_rdoq(S, p, k, S.luma_scan(e->rdModeList[c0 + i])) > 0);
    }
    HM_SYNC();
    // ---- reconstruction + distortion of every candidate, lanes on the samples
    for (int i = 0; i < nb; i++) {
      const int slot = i + (keep >= 0 && i >= keep), mode = HM_UNI(e->rdModeList[c0 + i]), cbf = HM_UNI(S.out_cbf(slot));
      simt_dequant_inv1(S, p, S.luma_scan(mode), slot, cbf, (TCoeff *)0);
      uint32_t sse = 0;
      simt_inv2_recon(S, bitDepth, cbf, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, N, L2, x, y, dcVal, bitDepth); },
                      [&](int x, int y, int r) HM_LAMBDA_INL { const int d = org[y * ps + x] - r; sse += (uint32_t)((d * d) >> shiftSse); });
      const uint32_t dist = hm_wave_sum(sse);
      if (hm_lane() == 0) S.out_dist(slot) = dist;
      HM_SYNC();
    }
    // ---- bits and cost of every candidate, one per lane (xGetIntraBitsQT :1038)
    HM_WAVE_FOR(k) {
      const int i = (keep >= 0 && k > keep) ? k - 1 : k;
      if ((ONE || k < JOBS) && k != keep && i < nb) {
        const int mode = e->rdModeList[c0 + i], cbf = S.out_cbf(k);
        uint32_t frac = commonFrac;
        simt_luma_mode_bits(e, S, k, &frac, mode);
        simt_bin(e, S, k, &frac, SimtDim<L2>::X_CBF, cbf);
        if (cbf) simt_code_coeff(e, S, k, k, 0, S.luma_scan(mode), &frac);
        S.out_frac(k) = frac;
        S.out_cost(k) = calc_rd_cost(e, frac >> 15, S.out_dist(k));
      }
    }
    HM_SYNC();
    int slotBest = keep;
    for (int i = 0; i < nb; i++) {                                 // the reference's comparison, in list order: the best so far came earlier in the list
      const int slot = i + (keep >= 0 && i >= keep); const double v = S.out_cost(slot);
      if (v < bestCost) { bestCost = v; slotBest = slot; best = c0 + i; }
    }
    kept = HM_UNI(slotBest); best = HM_UNI(best);
    c0 += nb;
#ifdef HM355_HOSTSIM
    batchesRun++;
#endif
  }
#ifdef HM355_HOSTSIM
  { const int top = L2 == 3 ? 11 : 7; g_first_pass_stats.cand[L2 - 3][numModes < top ? numModes : top]++; g_first_pass_stats.batches[L2 - 3][batchesRun < 3 ? batchesRun : 3]++; }
#endif
  const int bestMode = HM_UNI(e->rdModeList[best]);
  e->s8Winner = kept | (best << 8);
  HM_SYNC();
  return bestMode;
}

// The closing pass of estIntraPredQT (:2566-2600) starts with the unsplit evaluation of the winner's transform block -- the very evaluation the
// first pass made for it, from the same snapshot.  Instead of repeating it (xIntraCodingTUBlock + xGetIntraBitsQT), the winner's results are put
// where the residual quadtree expects them: levels and reconstruction in the layer buffers of the block's size and in the picture, the estimator
// (e->cur) advanced past the block's syntax (the bins every candidate codes alike, then the contexts and the bit count of the winner's lane).
// Must run right after the first pass (the overlays and the reference lines are still in place), with e->cur holding the CU's entry snapshot.
// Distortion / bits / cbf in e->outDistY / e->outBits / e->outDist.
template <int L2> HM_DEV HM_NOINLINE void simt_luma_winner_as_single_tu(Shared *e, TU tv)
{
  HM_ENTRY(e); tv = hm_uni_struct(tv);
  const TU *t = &tv; WorkSpace *ws = e->ws;
  const Simt<L2> S(e);
  const int won = HM_UNI(e->s8Winner), best = won & 255, z = t->cuZ + t->relZ, ps = e->stride[0], bitDepth = e->bitDepth;
  const int mode = HM_UNI(e->rdModeList[won >> 8]), cbf = HM_UNI(S.out_cbf(best));
  const SimtPar p = simt_params<L2>(e, 0);
  const int dcVal = ref_dc_val(e, 0, 1 << L2);
  Pel *rq = ws->qtRec[5 - L2] + t->y * 64 + t->x;
  Pel *recPic = e->fb.rec[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
  simt_dequant_inv1(S, p, S.luma_scan(mode), best, cbf, ws->qtCoef[5 - L2] + z * 16);
  simt_inv2_recon(S, bitDepth, cbf, [&](int x, int y) HM_LAMBDA_INL { return pred_sample(e, mode, 1 << L2, L2, x, y, dcVal, bitDepth); },
                  [&](int x, int y, int rr) HM_LAMBDA_INL { rq[y * 64 + x] = (Pel)rr; recPic[y * ps + x] = (Pel)rr; });
  HM_SYNC();
  { // the estimator: the bins in front of the lane's own (same as the first pass counted), then the lane's contexts and bit count
    CabacR r; cabr_load(e, r, &e->cur);
    simt_luma_common_bins<L2>(e, &r, t->cuZ);
    cabr_store(r, &e->cur);
  }
  simt_store_contexts(S, best, &e->cur, 1);
  e->cur.frac = (uint64_t)S.out_frac(best);
  e->outDistY = S.out_dist(best); e->outBits = S.out_frac(best) >> 15; e->outDist = (uint32_t)cbf;
  HM_SYNC();
}
