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
//   KEEPS_COST, keep_cost(), cost_at()       whether RDOQ stores the cost of each decided level (4x4) or prices it again (8x8)
// Then the small derivations the entry points have in common.  Included from hm355_core.h in front of the two.
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
