// hm355 -- candidates in lanes: independent 4x4 transform blocks evaluated one per lane.
//
// The reference tries the RD candidates of a prediction unit one after the other, each from the same CABAC snapshot
// (TEncSearch::estIntraPredQT :2473-2490, the transform-skip trial of xRecurIntraCodingQT :1452-1530, the five chroma
// modes of estIntraPredChromaQT :2740-2800).  None of them reads what another one wrote, so for 4x4 blocks -- where one
// candidate is far too little work for 64 lanes and where most of the evaluations of a CTU are -- the wavefront takes a
// whole candidate list at once: lane k owns candidate k from the prediction to the bit count (prediction, residual,
// DST/DCT or transform skip, RDOQ, de-quantisation, inverse transform, reconstruction, SSE, CABAC bit estimate), in the
// reference's arithmetic and operation order.  The decision among the candidates afterwards is the reference's
// sequential comparison (strict "<", first candidate wins ties) on the per-lane costs.
//
// Per-lane state lives in registers (the 16 samples / coefficients of the block) and in small lane-indexed LDS arrays
// that overlay the transform buffers, which are idle meanwhile.  The serial chains (tables of a batch, RDOQ, bit count of the
// coefficients) are the per-lane coefficient coder of hm355_simt.h at L2 = 2.  Included from hm355_core.h after it.
#pragma once

#define HM_SL 22                          // jobs (lanes in use) per batch: 11 luma candidates x {transform, transform skip}
struct Simt4A {                           // overlays Shared::bufA
  double cost[16][HM_SL];                 // RDOQ: cost of the level decided at each scan position
  double outCost[HM_SL];
  uint32_t outDist[HM_SL], outBits[HM_SL];
  int32_t tab[SimtDim<2>::T_N];           // bit costs of the batch's start state
  uint8_t ctx[SimtDim<2>::NCTX][HM_SL];   // context states of each job
  uint8_t outCbf[HM_SL];
  uint8_t lps[128];                       // LPS transitions
};
struct Simt4B {                           // overlays Shared::u behind the reference sample lines (RefLds::refMain onwards)
  int32_t cs[16][HM_SL];                  // coefficients in scan order
  int32_t dc[16][HM_SL];                  // level at decision time (low half) | final signed level (high half), scan order
  uint8_t scan[3][16];                    // scan position -> raster position of the three 4x4 scans
  uint8_t sigIdx[3][16];                  // scan position -> significance context increment
};
static_assert(sizeof(Simt4A) <= sizeof(((Shared *)0)->bufA), "Simt4A overlays bufA");
static_assert(offsetof(RefLds, refMain) + sizeof(Simt4B) <= sizeof(((Shared *)0)->u), "Simt4B overlays the tail of the LDS union");
static_assert(offsetof(RefLds, refMain) % 8 == 0, "alignment of the overlay");
// the three 4x4 coefficient scans (TComRom.cpp:140-225; checked against the generated tables by Simt<2>::load_scans in the host twin) and their inverses
HM_DEV constexpr int s4_scan(int type, int i)
{
  constexpr uint8_t t[3][16] = { {0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
                                 {0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15} };
  return t[type][i];
}
HM_DEV constexpr int s4_inv_scan(int type, int r)
{
  constexpr uint8_t t[3][16] = { {0, 2, 5, 9, 1, 4, 8, 12, 3, 7, 11, 14, 6, 10, 13, 15}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
                                 {0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15} };
  return t[type][r];
}
template <> struct Simt<2> {              // a batch of 4x4 blocks: RDOQ keeps the cost of each decided level, the significance increments are tabulated
  enum { JOBS = HM_SL, KEEPS_COST = 1 };
  Simt4A *A; Simt4B *B;
  HM_FINL_M explicit Simt(Shared *e) : A((Simt4A *)e->bufA), B((Simt4B *)((char *)&e->u + offsetof(RefLds, refMain))) {}
  HM_FINL_M uint8_t &out_cbf(int k) const { return A->outCbf[k]; }
  HM_FINL_M uint32_t &out_dist(int k) const { return A->outDist[k]; }
  HM_FINL_M uint32_t &out_frac(int k) const { return A->outBits[k]; }        // where a job keeps its Q15 count (simt_pick_chroma_mode)
  HM_FINL_M double &out_cost(int k) const { return A->outCost[k]; }
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
  HM_FINL_M int cs(int sp, int k) const { return B->cs[sp][k]; }
  HM_FINL_M int cg_pos(int, int) const { return 0; }
  HM_FINL_M int sig_inc(int scanType, int, int, int sp, int) const { return B->sigIdx[scanType][sp]; }
  HM_FINL_M void keep_cost(int sp, int k, double c) const { A->cost[sp][k] = c; }
  HM_FINL_M double cost_at(int sp, int k) const { return A->cost[sp][k]; }
  HM_FINL_M void load_scans(const Shared *e) const
  {
    HM_PAR_FOR(i, 48) {
      const int ty = i >> 4, sp = i & 15, blk = e->tab->scan[ty][0][sp];
      B->scan[ty][sp] = (uint8_t)blk; B->sigIdx[ty][sp] = HM_CTX_IND_MAP_4x4[blk];
#ifdef HM355_HOSTSIM
      if (blk != s4_scan(ty, sp) || s4_inv_scan(ty, blk) != sp) abort();   // the constexpr scans must equal the generated tables
#endif
    }
  }
};
typedef Simt<2> Simt4;

// one predicted sample of a 4x4 block of component type `chroma` from the unfiltered reference lines in slot `rs` of RefLds
HM_FINL int s4_pred_sample(const Shared *e, int rs, int chroma, int mode, int x, int y, int dcVal, int bitDepth)
{ return intra_pred_sample(e->u.ref.refTop[rs], e->u.ref.refLeft[rs], 4, 2, !chroma, mode, x, y, dcVal, bitDepth); }

// 4-point core transforms of one block held by one lane (xTrMxN / xITrMxN, TComTrQuant.cpp:836-935; DST for intra luma)
HM_FINL int s4_tm(int dst, int k, int j)
{
  if (dst) return HM_DST4[k * 4 + j];
  const int m = (k * 8 * (2 * j + 1)) & 127;      // the row k * 8 of the 32-point matrix (load_tmat)
  if (m <= 32) return HM_DCT_C[m]; if (m <= 64) return -HM_DCT_C[64 - m]; if (m <= 96) return -HM_DCT_C[m - 64]; return HM_DCT_C[128 - m];
}
HM_FINL void s4_fwd(int32_t *blk, int dst, int bitDepth)
{
  const int s1 = 2 + bitDepth + 6 - 15, a1 = 1 << (s1 - 1), s2 = 8, a2 = 128;
  int32_t t[16];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < 4; k++) { int32_t acc = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) acc += s4_tm(dst, k, i) * blk[j * 4 + i];
      t[k * 4 + j] = (acc + a1) >> s1; }
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int k = 0; k < 4; k++) { int32_t acc = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) acc += s4_tm(dst, k, i) * t[j * 4 + i];
      blk[k * 4 + j] = (acc + a2) >> s2; }
}
HM_FINL void s4_inv(int32_t *blk, int dst, int bitDepth)
{
  const int s1 = 7, s2 = 20 - bitDepth;
  int32_t t[16];
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int i = 0; i < 4; i++) { int32_t acc = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) acc += s4_tm(dst, k, i) * blk[k * 4 + j];
      t[j * 4 + i] = hm_clip3(-32768, 32767, (acc + (1 << (s1 - 1))) >> s1); }
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int i = 0; i < 4; i++) { int32_t acc = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) acc += s4_tm(dst, k, i) * t[k * 4 + j];
      blk[j * 4 + i] = hm_clip3(-32768, 32767, (acc + (1 << (s2 - 1))) >> s2); }
}

// the coefficient bits of a 4x4 block: its transform-skip flag (codeTransformSkipFlags :988), then codeCoeffNxN
HM_FINL void s4_code_coeff(const Shared *e, const Simt4 &S, int k, int src, int chroma, int scanType, int tskipFlag, uint32_t *frac)
{
  simt_bin(e, S, k, frac, SimtDim<2>::X_TSKIP, tskipFlag);
  simt_code_coeff(e, S, k, src, chroma, scanType, frac);
}

// lane arrays: a small array per lane (registers on the device; the host twin keeps one per emulated lane)
#ifdef HM355_HOSTSIM
#define HM_LVA(T, name, n) T name[64][n]
#define HM_LVAK(name, k) name[k]
#else
#define HM_LVA(T, name, n) T name[n]
#define HM_LVAK(name, k) name
#endif

// Prediction, residual, transform (or transform skip), RDOQ, reconstruction and distortion of job k's 4x4 block.
//   rs: reference line slot; org/ps: original block; mode: prediction mode; ts: transform skip; scanType: coefficient scan
// Leaves the reconstruction in rec[16], the levels (raster order) in lv[16]; returns the distortion, *cbf = coded block flag.
HM_FINL uint32_t s4_eval(Shared *e, const Simt4 &S, const SimtPar &p, int k, int rs, const Pel *org, int ps, int mode, int ts, int scanType,
                               int dcVal, int32_t *rec, int32_t *lv, int *cbf)
{
  int32_t pred[16], blk[16];
#pragma unroll
  for (int i = 0; i < 16; i++) {
    pred[i] = s4_pred_sample(e, rs, p.chroma, mode, i & 3, i >> 2, dcVal, p.bitDepth);
    const int r = org[(i >> 2) * ps + (i & 3)] - pred[i];
    blk[i] = ts ? r * (1 << p.tshift) : r;                            // xTransformSkip, TComTrQuant.cpp:1874
  }
  if (!ts) s4_fwd(blk, !p.chroma, p.bitDepth);
#pragma unroll
  for (int i = 0; i < 16; i++)                                      // into scan order (the lane's own scan)
    S.B->cs[i][k] = scanType == SCAN_HOR ? blk[s4_scan(SCAN_HOR, i)] : (scanType == SCAN_VER ? blk[s4_scan(SCAN_VER, i)] : blk[s4_scan(SCAN_DIAG, i)]);
  const int absSum = simt_rdoq(S, p, k, scanType);
  *cbf = absSum > 0;
#pragma unroll
  for (int i = 0; i < 16; i++) lv[i] = 0;
  if (absSum > 0) {
    int32_t ls[16];
#pragma unroll
    for (int i = 0; i < 16; i++) ls[i] = S.B->dc[i][k] >> 16;
#pragma unroll
    for (int j = 0; j < 16; j++)                                    // back to raster order
      lv[j] = scanType == SCAN_HOR ? ls[s4_inv_scan(SCAN_HOR, j)] : (scanType == SCAN_VER ? ls[s4_inv_scan(SCAN_VER, j)] : ls[s4_inv_scan(SCAN_DIAG, j)]);
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = simt_dequant(p, lv[i]);
    if (!ts) s4_inv(blk, !p.chroma, p.bitDepth);
    else {
      const int off = p.tshift == 0 ? 0 : (1 << (p.tshift - 1));
#pragma unroll
      for (int i = 0; i < 16; i++) blk[i] = (int16_t)((blk[i] + off) >> p.tshift);      // xITransformSkip, :1920 (stored as Pel)
    }
  } else {
#pragma unroll
    for (int i = 0; i < 16; i++) blk[i] = 0;
  }
  const int maxv = (1 << p.bitDepth) - 1, shiftSse = (p.bitDepth - 8) << 1;
  uint32_t sse = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const int r = hm_clip3(0, maxv, pred[i] + (int16_t)blk[i]);
    rec[i] = r;
    const int d = org[(i >> 2) * ps + (i & 3)] - r; sse += (uint32_t)((d * d) >> shiftSse);
  }
  return sse;
}

// ------------------------------------------------------------------------------------------------
// luma: the RD candidates of one 4x4 prediction unit of an NxN CU (the candidate loop of estIntraPredQT :2473-2560 with the
// transform-skip trial of xRecurIntraCodingQT inside), all at once.  e->cur holds the CU's entry snapshot (CI_CURR_BEST);
// e->u.ref the PU's reference samples; e->rdModeList[0..numModes) the candidates; e->mpmPreds the PU's most probable modes.
// Writes the winner's decision (tr / cbf / ts / dirL of the partition, coefficients, reconstruction into ws->reco) and
// returns its mode / distortion / cost in e->outBits / e->outDistY / e->outRdCost.
// ------------------------------------------------------------------------------------------------
HM_DEV HM_NOINLINE void simt4_luma_pu(Shared *e, TU tv, int numModes)
{
  HM_ENTRY(e); numModes = HM_UNI(numModes); tv = hm_uni_struct(tv);
  const TU *t = &tv; CtuMeta *m = (&e->meta); WorkSpace *ws = e->ws;
  const int z = t->cuZ + t->relZ, ps = e->stride[0], jobs = 2 * numModes;
  // bits every candidate spends before its own bins (xEncIntraHeader :965-1032 for the first PU of the CU): same contexts, same
  // values for all of them; none of those contexts is touched again inside the block
  uint32_t commonFrac;
  {
    CabacR r; cabr_load(e, r, &e->cur);
    r.frac &= 32767;
    if (t->relZ == 0) {
      if (e->im) { code_skip_flag(e, &r, t->cuZ); enc_bin(e, &r, C_PRED_MODE, 1); }
      if (t->cuDepth == 3) enc_bin(e, &r, C_PART, 0);
    }
    commonFrac = (uint32_t)r.frac;
  }
  const Simt4 S(e); Simt4A *A = S.A;
  simt_setup(e, S, &e->cur, jobs, 0, 0, 0, C_INTRA_LUMA);          // luma cbf of a TU below the CU root: context 0 (code_qt_cbf)
  const SimtPar p = simt_params<2>(e, 0);
  const Pel *org = e->fb.org[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
  const int dcVal = ref_dc_val(e, 0, 4);
  HM_LVA(int32_t, rec, 16); HM_LVA(int32_t, lv, 16);
  HM_WAVE_FOR(k) {
    if (k < jobs) {
      const int mode = e->rdModeList[k >> 1], ts = k & 1, scanType = intra_scan_type(mode);      // getCoefScanIdx (4x4 intra luma)
      int cbf;
      const uint32_t dist = s4_eval(e, S, p, k, 0, org, ps, mode, ts, scanType, dcVal, HM_LVAK(rec, k), HM_LVAK(lv, k), &cbf);
      // bits: xGetIntraBitsQT :1038 = prediction mode (codeIntraDirLumaAng :636), cbf, coefficients
      uint32_t frac = commonFrac;
      simt_luma_mode_bits(e, S, k, &frac, mode);
      simt_bin(e, S, k, &frac, SimtDim<2>::X_CBF, cbf);
      if (cbf) s4_code_coeff(e, S, k, k, 0, scanType, ts, &frac);
      const uint32_t bits = frac >> 15;
      A->outDist[k] = dist; A->outBits[k] = bits; A->outCbf[k] = (uint8_t)cbf;
      A->outCost[k] = calc_rd_cost(e, bits, dist);
    }
  }
  HM_SYNC();
  // the reference's sequential decision: transform skip against the transform (xRecurIntraCodingQT :1452-1530), then candidate
  // against candidate (estIntraPredQT :2520-2560); strict "<" throughout
  double bestCost = HM_MAX_DOUBLE; int bestJob = 0;
  for (int c = 0; c < numModes; c++) {
    double single = A->outCost[2 * c]; int pick = 2 * c;
    if (A->outCbf[2 * c + 1]) { const double c1 = A->outCost[2 * c + 1]; if (c1 < single) { single = c1; pick = 2 * c + 1; } }
    if (single < bestCost) { bestCost = single; bestJob = pick; }
  }
  bestJob = HM_UNI(bestJob);
  const int bestMode = e->rdModeList[bestJob >> 1], bestCbf = A->outCbf[bestJob];
  e->outBits = (uint32_t)bestMode; e->outDistY = A->outDist[bestJob]; e->outRdCost = bestCost;
  HM_WAVE_FOR(k) {
    if (k == bestJob) {
      TCoeff *coef = e->cc + z * 16; Pel *ro = ws->reco + t->y * 64 + t->x;
#pragma unroll
      for (int i = 0; i < 16; i++) { coef[i] = HM_LVAK(lv, k)[i]; ro[(i >> 2) * 64 + (i & 3)] = (Pel)HM_LVAK(rec, k)[i]; }
    }
  }
  if (hm_lane() == 0) {
    m->tr[z] = (uint8_t)t->trDepth; m->cbf[0][z] = (uint8_t)(bestCbf << t->trDepth); m->ts[0][z] = (uint8_t)(bestJob & 1); m->dirL[z] = (uint8_t)bestMode;
  }
  HM_SYNC();
}

// ------------------------------------------------------------------------------------------------
// chroma of an 8x8 CU: its one 4x4 block per component under the five chroma modes (estIntraPredChromaQT :2698-2849 over
// xRecurIntraChromaCodingQT :1958-2145), ten evaluations at once: job 2 * modeIndex + (component - 1).  None of them codes a
// bin before the mode's bits are counted, so all start from the CU's entry snapshot in e->cur.  Then one lane per mode counts
// the mode's bits on its own context copy, and the modes are compared in the reference's order (simt_pick_chroma_mode,
// hm355_simt.h, with the 4x4 coder and the mode's scan).  `leaf`: the TU that carries the chroma blocks (the CU's
// root TU, or its first 4x4 luma quadrant when the luma transform is split).  Not used when that TU tries transform skip
// (chroma_tu: the Cr trial then starts from the contexts the Cb winner left, so the evaluations chain).
// Writes the winner (dirC / cbf / ts of the CU, coefficients, reconstruction into ws->reco) and returns its distortion.
// ------------------------------------------------------------------------------------------------
HM_DEV HM_NOINLINE uint32_t simt4_chroma_cu(Shared *e, TU leafv, int cuZ)
{
  HM_ENTRY(e); cuZ = HM_UNI(cuZ); leafv = hm_uni_struct(leafv);
  const TU *t = &leafv; CtuMeta *m = (&e->meta); WorkSpace *ws = e->ws;
  const int zc = t->cuZ + t->cRelZ, r = hm_z2r(zc);
  const int x4 = e->ctuX * 16 + (r & 15), y4 = e->ctuY * 16 + (r >> 4), px = e->ctuX * 32 + t->cx, py = e->ctuY * 32 + t->cy;
  simt_chroma_ref_lines(e, px, py, 4, x4, y4);
  int modeList[5];
  const int lumaDir = m->dirL[cuZ];
  allowed_chroma_dirs(lumaDir, modeList);
  const Simt4 S(e); Simt4A *A = S.A;
  simt_setup(e, S, &e->cur, 10, 1, 5 + t->trDepth, 5, C_CHROMA_PRED);
  const SimtPar p = simt_params<2>(e, 1);
  const uint32_t baseFrac = (uint32_t)(e->cur.frac & 32767);
  const int dcVal[2] = { ref_dc_val(e, 0, 4), ref_dc_val(e, 1, 4) };
  HM_LVA(int32_t, rec, 16); HM_LVA(int32_t, lv, 16);
  HM_WAVE_FOR(k) {
    if (k < 10) {
      const int c = k & 1, mi = k >> 1, ps = e->stride[1 + c];
      const int dirC = chroma_mode_at(modeList, mi), mode = dirC == DM_CHROMA_IDX ? lumaDir : dirC, scanType = intra_scan_type(mode);      // getCoefScanIdx (4x4 intra chroma)
      const Pel *org = e->fb.org[1 + c] + (size_t)py * ps + px;
      int cbf;
      const uint32_t sse = s4_eval(e, S, p, k, c, org, ps, mode, 0, scanType, c ? dcVal[1] : dcVal[0], HM_LVAK(rec, k), HM_LVAK(lv, k), &cbf);
      A->outDist[k] = (uint32_t)(e->fb.chromaWeight * (double)sse);   // getDistPart, TComRdCost.cpp:447-450
      A->outCbf[k] = (uint8_t)cbf;
    }
  }
  HM_SYNC();
  const int best = simt_pick_chroma_mode(e, S, baseFrac, modeList, [&](int k, int src, uint32_t *frac) HM_LAMBDA_INL {
    const int dirC = chroma_mode_at(modeList, k >> 1);
    s4_code_coeff(e, S, k, src, 1, intra_scan_type(dirC == DM_CHROMA_IDX ? lumaDir : dirC), 0, frac);
  });
  const uint32_t bestDist = A->outDist[2 * best] + A->outDist[2 * best + 1];
  const int cbfU = A->outCbf[2 * best], cbfV = A->outCbf[2 * best + 1];
  HM_WAVE_FOR(k) {
    if ((k >> 1) == best && k < 10) {
      const int po = HM_PLANE_OFF(1 + (k & 1));
      TCoeff *coef = e->cc + po + t->cOff; Pel *ro = ws->reco + po + t->cy * 32 + t->cx;
#pragma unroll
      for (int i = 0; i < 16; i++) { coef[i] = HM_LVAK(lv, k)[i]; ro[(i >> 2) * 32 + (i & 3)] = (Pel)HM_LVAK(rec, k)[i]; }
    }
  }
  { // decision arrays of the CU: cbf at the leaf's depth, merged into depth 0 when the luma transform is split (xRecurIntraChromaCodingQT :2120-2140)
    const int vU = t->trDepth ? 3 * cbfU : cbfU, vV = t->trDepth ? 3 * cbfV : cbfV, bm = chroma_mode_at(modeList, best);
    HM_PAR_FOR(i, 4) { m->cbf[1][cuZ + i] = (uint8_t)vU; m->cbf[2][cuZ + i] = (uint8_t)vV; m->ts[1][cuZ + i] = 0; m->ts[2][cuZ + i] = 0; m->dirC[cuZ + i] = (uint8_t)bm; }
  }
  simt_store_chroma_mode(S, 2 * best, &e->cur, S.out_frac(2 * best));      // e->cur: the estimator after the winning mode's count
  HM_SYNC();
  return bestDist;
}

// ------------------------------------------------------------------------------------------------
// One 4x4 luma transform block inside a residual quadtree (xIntraCodingTUBlock :1074 + xGetIntraBitsQT :1038 of a leaf of
// xRecurIntraCodingQT, no transform-skip trial: 2Nx2N CUs).  Nothing runs beside it -- the blocks of a quadtree chain through the
// reconstruction and the CABAC state -- but for a block this small the per-lane form of the evaluation (hm355_simt4.h) on ONE lane
// is shorter than the wave-uniform form with its 64-lane staging and its LDS / HBM round trips, so it runs there.  Side effects
// are those of the two reference functions: coefficients and reconstruction in the quadtree layer buffers and the picture,
// tr / cbf of the partition, the estimator (e->cur) advanced past the block's syntax.  Distortion / bits in e->outDistY / e->outBits.
// ------------------------------------------------------------------------------------------------
HM_DEV HM_NOINLINE void simt4_luma_leaf(Shared *e, TU tv)
{
  HM_ENTRY(e); tv = hm_uni_struct(tv);
  const TU *t = &tv; CtuMeta *m = (&e->meta); WorkSpace *ws = e->ws;
  const int z = t->cuZ + t->relZ, ps = e->stride[0], r = hm_z2r(z), mode = m->dirL[z];
  init_adi_pattern(e, 0, e->ctuX * 64 + t->x, e->ctuY * 64 + t->y, 4, e->ctuX * 16 + (r & 15), e->ctuY * 16 + (r >> 4), 1, 0);
  { // the bins in front of the block's own (xEncIntraHeader :965), on the estimator itself
    CabacR cr; cabr_load(e, cr, &e->cur);
    cr.frac &= 32767;
    enc_intra_header(e, &cr, t, 1, 0);
    cabr_store(cr, &e->cur);
  }
  const Simt4 S(e); Simt4A *A = S.A;
  simt_setup(e, S, &e->cur, 1, 0, 0, 0, C_INTRA_LUMA);             // luma cbf below the CU's root TU: context 0
  const SimtPar p = simt_params<2>(e, 0);
  const Pel *org = e->fb.org[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
  const int dcVal = ref_dc_val(e, 0, 4);
  const int scanType = intra_scan_type(mode);
  const uint32_t frac0 = (uint32_t)e->cur.frac;
  HM_WAVE_FOR(k) {
    if (k == 0) {
      int32_t rec[16], lv[16]; int cbf;
      const uint32_t dist = s4_eval(e, S, p, 0, 0, org, ps, mode, 0, scanType, dcVal, rec, lv, &cbf);
      uint32_t frac = frac0;
      simt_bin(e, S, 0, &frac, SimtDim<2>::X_CBF, cbf);             // xEncSubdivCbfQT :856: a 4x4 block codes no split flag
      if (cbf) s4_code_coeff(e, S, 0, 0, 0, scanType, 0, &frac);
      A->outDist[0] = dist; A->outBits[0] = frac; A->outCbf[0] = (uint8_t)cbf;
      TCoeff *coef = ws->qtCoef[3] + z * 16; Pel *rq = ws->qtRec[3] + t->y * 64 + t->x;
      Pel *recPic = e->fb.rec[0] + (e->ctuY * 64 + t->y) * ps + e->ctuX * 64 + t->x;
#pragma unroll
      for (int i = 0; i < 16; i++) { coef[i] = lv[i]; rq[(i >> 2) * 64 + (i & 3)] = (Pel)rec[i]; recPic[(i >> 2) * ps + (i & 3)] = (Pel)rec[i]; }
    }
  }
  HM_SYNC();
  // the estimator after the block: the contexts the lane advanced, the bit count
  simt_store_contexts(S, 0, &e->cur, 0);
  const int cbf = A->outCbf[0];
  e->cur.frac = (uint64_t)A->outBits[0];
  e->outDistY = A->outDist[0]; e->outBits = A->outBits[0] >> 15;
  if (hm_lane() == 0) { m->tr[z] = (uint8_t)t->trDepth; m->cbf[0][z] = (uint8_t)(cbf << t->trDepth); }
  HM_SYNC();
}

// The 4x4 chroma blocks (Cb, Cr) of one transform unit under the CU's current chroma mode, no transform-skip trial
// (xIntraCodingTUBlock :1074 twice, from xRecurIntraChromaCodingQT :1958): two independent evaluations from the same estimator
// state, one per lane.  Side effects as the reference function's; returns the sum of the weighted distortions.
HM_DEV HM_NOINLINE uint32_t simt4_chroma_leaf(Shared *e, TU tv)
{
  HM_ENTRY(e); tv = hm_uni_struct(tv);
  const TU *t = &tv; CtuMeta *m = (&e->meta); WorkSpace *ws = e->ws;
  const int zc = t->cuZ + t->cRelZ, r = hm_z2r(zc), layer = 5 - t->log2;
  const int x4 = e->ctuX * 16 + (r & 15), y4 = e->ctuY * 16 + (r >> 4), px = e->ctuX * 32 + t->cx, py = e->ctuY * 32 + t->cy;
  simt_chroma_ref_lines(e, px, py, 4, x4, y4);
  int mode = m->dirC[zc];
  if (mode == DM_CHROMA_IDX) mode = m->dirL[zc & ~3];
  const int scanType = intra_scan_type(mode);
  const Simt4 S(e); Simt4A *A = S.A;
  simt_setup(e, S, &e->cur, 2, 1, 5 + t->trDepth, 5, C_CHROMA_PRED);
  const SimtPar p = simt_params<2>(e, 1);
  const int dcVal[2] = { ref_dc_val(e, 0, 4), ref_dc_val(e, 1, 4) };
  HM_WAVE_FOR(k) {
    if (k < 2) {
      const int ps = e->stride[1 + k], po = HM_PLANE_OFF(1 + k);
      const Pel *org = e->fb.org[1 + k] + (size_t)py * ps + px;
      int32_t rec[16], lv[16]; int cbf;
      const uint32_t sse = s4_eval(e, S, p, k, k, org, ps, mode, 0, scanType, k ? dcVal[1] : dcVal[0], rec, lv, &cbf);
      A->outDist[k] = (uint32_t)(e->fb.chromaWeight * (double)sse);
      A->outCbf[k] = (uint8_t)cbf;
      TCoeff *coef = ws->qtCoef[layer] + po + t->cOff; Pel *rq = ws->qtRec[layer] + po + t->cy * 32 + t->cx;
      Pel *recPic = e->fb.rec[1 + k] + (size_t)py * ps + px;
#pragma unroll
      for (int i = 0; i < 16; i++) { coef[i] = lv[i]; rq[(i >> 2) * 32 + (i & 3)] = (Pel)rec[i]; recPic[(i >> 2) * ps + (i & 3)] = (Pel)rec[i]; }
    }
  }
  HM_SYNC();
  const int cbfU = A->outCbf[0], cbfV = A->outCbf[1];
  const uint32_t dist = A->outDist[0] + A->outDist[1];
  HM_PAR_FOR(i, t->cParts) { m->cbf[1][zc + i] = (uint8_t)(cbfU << t->trDepth); m->cbf[2][zc + i] = (uint8_t)(cbfV << t->trDepth); m->ts[1][zc + i] = 0; m->ts[2][zc + i] = 0; }
  HM_SYNC();
  return dist;
}
