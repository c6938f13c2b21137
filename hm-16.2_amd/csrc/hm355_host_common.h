// Host-side helpers shared by the HIP library (hm355_capi.hip) and the host simulation used for
// debugging (tests/hostsim): lookup-table generation, slice parameter derivation, CTU scheduling.
#pragma once
#include "hm355_types.h"
#include <math.h>
#include <string.h>
#include <vector>

// z-scan <-> raster of the 16x16 grid of 4x4 partitions (TComRom.cpp:256-290) and the coefficient
// scans (ScanGenerator, TComRom.cpp:52-225)
static inline void hm355_gen_scan(int w, int h, int stride, int type, int offx, int offy, uint16_t *out, int count)
{
  int line = 0, col = 0;
  for (int i = 0; i < count; i++) {
    out[i] = (uint16_t)((line + offy) * stride + col + offx);
    if (type == 0) {
      if (col == w - 1 || line == 0) { line += col + 1; col = 0; if (line >= h) { col += line - (h - 1); line = h - 1; } }
      else { col++; line--; }
    } else if (type == 1) { if (col == w - 1) { line++; col = 0; } else col++; }
    else { if (line == h - 1) { col++; line = 0; } else line++; }
  }
}
static inline void hm355_build_tables(Tables *t)
{
  memset(t, 0, sizeof(*t));
  for (int z = 0; z < 256; z++) { // bit de-interleave: z-scan index -> (x,y)
    int x = 0, y = 0;
    for (int b = 0; b < 4; b++) { x |= ((z >> (2 * b)) & 1) << b; y |= ((z >> (2 * b + 1)) & 1) << b; }
    t->z2r[z] = (uint8_t)(y * 16 + x); t->r2z[y * 16 + x] = (uint8_t)z;
  }
  for (int ty = 0; ty < 3; ty++)
    for (int l = 0; l < 4; l++) {
      const int n = 4 << l, g = n >> 2;
      hm355_gen_scan(g, g, g, ty, 0, 0, t->scanCG[ty][l], g * g);
      for (int gi = 0; gi < g * g; gi++) {
        const int gx = t->scanCG[ty][l][gi] % g, gy = t->scanCG[ty][l][gi] / g;
        hm355_gen_scan(4, 4, n, ty, gx * 4, gy * 4, t->scan[ty][l] + gi * 16, 16);
      }
    }
}

static const uint8_t HM355_CHROMA_SCALE_420[58] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9,10,11,12,13,14,15,16,17,18,19,20,21,22,23,24,25,26,27,28,29,29,30,31,32,33,33,34,34,35,35,36,36,37,37,38,39,40,41,42,43,44,45,46,47,48,49,50,51 };

// what TEncSlice::setUpLambda (TEncSlice.cpp:132-159), QpParam (TComTrQuant.cpp:71-119),
// setErrScaleCoeff (:2933-2956) and the sign-hiding factor (:2382-2386) derive from (qp, lambda, weight)
static inline void hm355_fill_slice_params(FrameBuf *f, int bitDepth, int qp, double lambda, double chromaWeight)
{
  static const int quantScales[6] = {26214, 23302, 20560, 18396, 16384, 14564};
  static const int invQuantScales[6] = {40, 45, 51, 57, 64, 72};
  f->qp = qp; f->lambda = lambda; f->sqrtLambda = sqrt(lambda); f->chromaWeight = chromaWeight; f->lambdaC = lambda / chromaWeight;
  const int bdOff = 6 * (bitDepth - 8);
  const int q = qp + bdOff; f->qpPer[0] = q / 6; f->qpRem[0] = q % 6;
  int qc = qp < -bdOff ? -bdOff : (qp > 57 ? 57 : qp);
  qc = (qc < 0) ? qc + bdOff : HM355_CHROMA_SCALE_420[qc] + bdOff;
  f->qpPer[1] = qc / 6; f->qpRem[1] = qc % 6;
  for (int ch = 0; ch < 2; ch++) {
    for (int l = 0; l < 4; l++) {
      const int transformShift = 15 - bitDepth - (l + 2);
      double errScale = (double)(1 << 15);
      errScale = errScale * pow(2.0, -2.0 * transformShift);
      errScale = errScale / quantScales[f->qpRem[ch]] / quantScales[f->qpRem[ch]] / (double)(1 << (2 * (bitDepth - 8)));
      f->errScale[ch][l] = errScale;
    }
    const double lam = ch ? f->lambdaC : f->lambda;
    const double invQ = (double)invQuantScales[f->qpRem[ch]];
    f->rdFactor[ch] = (int64_t)(invQ * invQ * (double)(1 << (2 * f->qpPer[ch])) / lam / 16 / (double)(1 << (2 * (bitDepth - 8))) + 0.5);
  }
}

// cu_qp_delta: the quantiser state of every QP a coding unit may take (-12..51, entry q + 12 of DqpPic::tab) under the slice's lambda and chroma weight
static inline void hm355_fill_qp_tab(QpTab tab[64], int bitDepth, double lambda, double chromaWeight)
{
  for (int q = -12; q <= 51; q++) {
    FrameBuf t; memset(&t, 0, sizeof(t));
    hm355_fill_slice_params(&t, bitDepth, q, lambda, chromaWeight);
    QpTab &e = tab[q + 12];
    for (int k = 0; k < 2; k++) { e.qpPer[k] = t.qpPer[k]; e.qpRem[k] = t.qpRem[k]; e.rdFactor[k] = t.rdFactor[k]; for (int l = 0; l < 4; l++) e.errScale[k][l] = t.errScale[k][l]; }
  }
}

// LCU-level rate control: the record of one CTU -- what TComRdCost::setLambda (TComRdCost.cpp:194-216) and TComTrQuant::setLambdas with the
// slice's chroma weight (TEncSlice.cpp:793-803) derive from the lambda the rate model gives it, with the sign-hiding factor of its QP
static inline CtuRc hm355_ctu_rc_record(int bitDepth, int qp, double lambda, double chromaWeight)
{
  FrameBuf t; memset(&t, 0, sizeof(t));
  hm355_fill_slice_params(&t, bitDepth, qp, lambda, chromaWeight);
  CtuRc r; memset(&r, 0, sizeof(r));
  r.lambda = t.lambda; r.sqrtLambda = t.sqrtLambda; r.lambdaC = t.lambdaC; r.rdFactor[0] = t.rdFactor[0]; r.rdFactor[1] = t.rdFactor[1];
  r.lambdaMotionSAD = (uint32_t)floor(65536.0 * t.sqrtLambda); r.lambdaMotionSSE = (uint32_t)floor(65536.0 * lambda);
  return r;
}

// I-slice lambda of an all-intra GOP (TEncSlice::initEncSlice, TEncSlice.cpp:323-352) -- used by our
// TEncSlice look-alike and by the tests; the C ABI itself takes lambda from the caller.
static inline void hm355_intra_lambda(int qp, double *lambda, double *chromaWeight)
{
  *lambda = 0.57 * pow(2.0, ((double)qp - 12) / 3.0);
  const int q = qp < 0 ? 0 : (qp > 57 ? 57 : qp);
  const int qpc = HM355_CHROMA_SCALE_420[q];
  *chromaWeight = pow(2.0, (qp - qpc) / 3.0);
}

// ---- tiles (TComPicSym::initTiles and the address maps above it, TComPicSym.cpp:160-300) ----
#define HM_MAX_TILE_COLS 20   /* Table A.1: level 6.2 */
#define HM_MAX_TILE_ROWS 22
#define HM_MIN_TILE_COLS_CTU 4   /* Main / Main10: a tile is at least 256 luma samples wide and 64 high (TComPicSym.cpp:251-271) */
// uniform spacing: column c of n over w CTUs is (c + 1) * w / n - c * w / n CTUs wide; rows alike
static inline void hm355_tile_uniform_spacing(int wCtu, int hCtu, int cols, int rows, int *colWidth, int *rowHeight)
{
  for (int c = 0; c < cols; c++) colWidth[c] = (c + 1) * wCtu / cols - c * wCtu / cols;
  for (int r = 0; r < rows; r++) rowHeight[r] = (r + 1) * hCtu / rows - r * hCtu / rows;
}
struct hm355_tile_tables {
  int cols = 1, rows = 1;
  std::vector<int> colWidth, rowHeight;   // CTUs
  std::vector<int> firstCtu;              // [tile] raster address of its first CTU
  std::vector<int> tileOf;                // [raster address] tile index (tile row * cols + tile column)
  std::vector<int> rsToTs, tsToRs;        // raster address -> position in tile scan (coding order), and back
  std::vector<TileCtu> ctu;               // [raster address] what the device reads (Params::tile)
  int count() const { return cols * rows; }
};
// The tables of a layout of cols x rows tiles over wCtu x hCtu CTUs.  Returns NULL, or the reason the layout is refused (then `t` is untouched).
static inline const char *hm355_build_tiles(int wCtu, int hCtu, int cols, const int *colWidth, int rows, const int *rowHeight, hm355_tile_tables *t)
{
  if (cols < 1 || rows < 1 || !colWidth || !rowHeight) return "the layout needs one tile column and one tile row or more, with their widths and heights";
  if (cols > HM_MAX_TILE_COLS || rows > HM_MAX_TILE_ROWS) return "more than 20 tile columns or 22 tile rows";
  int sw = 0, sh = 0;
  for (int c = 0; c < cols; c++) { if (cols > 1 || rows > 1) if (colWidth[c] < HM_MIN_TILE_COLS_CTU) return "a tile column is narrower than 4 CTUs (256 luma samples)"; sw += colWidth[c]; }
  for (int r = 0; r < rows; r++) { if (rowHeight[r] < 1) return "a tile row is lower than 1 CTU"; sh += rowHeight[r]; }
  if (sw != wCtu) return "the tile column widths do not sum to the picture's width in CTUs";
  if (sh != hCtu) return "the tile row heights do not sum to the picture's height in CTUs";
  hm355_tile_tables o;
  o.cols = cols; o.rows = rows; o.colWidth.assign(colWidth, colWidth + cols); o.rowHeight.assign(rowHeight, rowHeight + rows);
  const int n = wCtu * hCtu;
  o.firstCtu.resize(cols * rows); o.tileOf.resize(n); o.rsToTs.resize(n); o.tsToRs.resize(n); o.ctu.resize(n);
  int ts = 0, last = -1;
  for (int r = 0, y0 = 0; r < rows; y0 += rowHeight[r], r++)
    for (int c = 0, x0 = 0; c < cols; x0 += colWidth[c], c++) {
      o.firstCtu[r * cols + c] = y0 * wCtu + x0;
      for (int y = y0; y < y0 + rowHeight[r]; y++)
        for (int x = x0; x < x0 + colWidth[c]; x++) {
          const int a = y * wCtu + x;
          TileCtu e; e.x0 = (int16_t)x0; e.x1 = (int16_t)(x0 + colWidth[c]); e.y0 = (int16_t)y0; e.y1 = (int16_t)(y0 + rowHeight[r]);
          e.prev = (x == x0 && y == y0) ? -1 : last; e.scanPrev = last;
          o.ctu[a] = e; o.tileOf[a] = r * cols + c; o.rsToTs[a] = ts; o.tsToRs[ts] = a;
          last = a; ts++;
        }
    }
  *t = o;
  return NULL;
}
// the first CTU of tile `tile` starts from the m_integerMv2Nx2N of the last CTU of the tile before it (process_ctu): its 64x64 CU crosses the picture edge
static inline int hm355_tile_carries(const hm355_tile_tables &t, int tile, int width, int height)
{
  if (tile == 0) return 0;
  const int c = tile % t.cols, r = tile / t.cols;
  int x0 = 0, y0 = 0;
  for (int i = 0; i < c; i++) x0 += t.colWidth[i];
  for (int i = 0; i < r; i++) y0 += t.rowHeight[i];
  return x0 * 64 + 63 >= width || y0 * 64 + 63 >= height;
}

// ---- slices (hm355_set_slices) ----
// SliceMode=1 (FIXED_NUMBER_OF_CTU), TEncSlice::calculateBoundingCtuTsAddrForSlice (TEncSlice.cpp:1097-1182) without tiles: a slice ends
// ctusPerSlice CTUs after its start or with the picture; under WaveFrontSynchro a slice that starts inside a CTU row ends with that row at the
// latest.  Returns the number of slices (0: bad arguments) and writes the first `cap` first CTUs.
static inline int hm355_slice_fixed_ctus(int wCtu, int hCtu, int wpp, int ctusPerSlice, int *firstCtu, int cap)
{
  if (wCtu < 1 || hCtu < 1 || ctusPerSlice < 1) return 0;
  const int n = wCtu * hCtu;
  int count = 0;
  for (int a = 0; a < n; count++) {
    if (firstCtu && count < cap) firstCtu[count] = a;
    int end = a + ctusPerSlice < n ? a + ctusPerSlice : n;
    if (wpp && a % wCtu != 0 && a - a % wCtu + wCtu < end) end = a - a % wCtu + wCtu;
    a = end;
  }
  return count;
}
struct hm355_slice_tables {
  std::vector<int> first;                 // [slice] raster address of its first CTU, ascending from 0
  std::vector<int> start;                 // `first`, then the number of CTUs (Params::sliceStart)
  std::vector<SliceCtu> ctu;              // [raster address] what the device reads (Params::slice)
  int count() const { return first.empty() ? 1 : (int)first.size(); }
};
// The tables of a partition into `num` slices over wCtu x hCtu CTUs.  Returns NULL, or the reason the partition is refused (then `t` is untouched).
static inline const char *hm355_build_slices(int wCtu, int hCtu, int wpp, int num, const int *firstCtu, hm355_slice_tables *t)
{
  const int n = wCtu * hCtu;
  if (num < 1 || !firstCtu) return "the partition needs one slice or more, with the first CTU of each";
  if (firstCtu[0] != 0) return "the first slice does not start at CTU 0";
  for (int k = 1; k < num; k++) if (firstCtu[k] <= firstCtu[k - 1]) return "the first CTUs are not ascending";
  if (firstCtu[num - 1] >= n) return "a slice starts past the picture";
  for (int k = 0; wpp && k < num; k++) {
    const int a = firstCtu[k], end = k + 1 < num ? firstCtu[k + 1] : n;
    if (a % wCtu != 0 && end > a - a % wCtu + wCtu) return "under WaveFrontSynchro a slice that starts inside a CTU row must end with that row";
  }
  hm355_slice_tables o;
  o.first.assign(firstCtu, firstCtu + num); o.start = o.first; o.start.push_back(n); o.ctu.resize(n);
  for (int k = 0; k < num; k++) for (int a = o.start[k]; a < o.start[k + 1]; a++) { o.ctu[a].first = o.start[k]; o.ctu[a].end = o.start[k + 1]; }
  *t = o;
  return NULL;
}
// the first CTU of slice k starts from the m_integerMv2Nx2N of the CTU before it (process_ctu): its 64x64 CU crosses the picture's right or bottom edge
static inline int hm355_slice_carries(const hm355_slice_tables &t, int k, int wCtu, int width, int height)
{
  if (k == 0) return 0;
  const int a = t.first[k];
  return (a % wCtu) * 64 + 63 >= width || (a / wCtu) * 64 + 63 >= height;
}

// Dependency-ordered launch schedule.  Step s holds every CTU whose inputs (left, above-left, above,
// above-right CTU and the CABAC hand-off) were produced in steps < s:
//   WaveFrontSynchro=1 : CTU (x,y) runs at step x + 2y   (2-CTU lag wavefront, TEncSlice.cpp:740-755)
//   WaveFrontSynchro=0 : the CABAC state chains through every CTU in raster order -> step = address
// All pictures of a batch are independent, so step s carries the CTUs of every picture.
// carryLastRow (inter slices under WPP whose last CTU row is cut by the picture edge): CTU (0, last row) also needs the
// 2Nx2N integer-MV state of the last CTU of the row above, so that row is ordered behind the whole row above it.
static inline int hm355_schedule_step(int wCtu, int hCtu, int wpp, int carryLastRow, int x, int y)
{
  if (!wpp) return y * wCtu + x;
  if (carryLastRow && hCtu > 1 && wCtu > 1 && y == hCtu - 1) return (wCtu - 1) + 2 * (hCtu - 2) + 1 + x;
  return x + 2 * y;
}
// Tiles (never with WaveFrontSynchro): every tile is a chain of its own, a CTU's step is its index inside its tile, and the tiles of a picture are
// interleaved like the pictures of a batch.  carryTiles (inter slices): a tile whose first CTU starts from the 2Nx2N integer-MV state of the last
// CTU of the tile before it (hm355_tile_carries; width, height: the picture's) is ordered behind that tile, as carryLastRow does for a WPP row.
static inline void hm355_build_schedule(int wCtu, int hCtu, int wpp, int nFrames, std::vector<WorkItem> &items, std::vector<int> &stepStart, int carryLastRow = 0,
                                        int firstFrame = 0, int firstCtu = 0, int lastCtu = -1, const hm355_tile_tables *tiles = NULL, int carryTiles = 0,
                                        int width = 0, int height = 0, const hm355_slice_tables *slices = NULL)
{ // CTUs [firstCtu, lastCtu] (raster addresses, i.e. coding order) of the pictures in slots [firstFrame, firstFrame + nFrames): a band of CTUs (the
  // CTUs before it are complete) -- whole CTU rows (hm355_run_rows), or any range (hm355_run_ctus)
  // slices (hm355_set_slices, without WaveFrontSynchro and without tiles): every slice is a chain of its own, exactly as every tile is; carryTiles
  // then orders a slice whose first CTU the picture edge cuts (hm355_slice_carries) behind the slice before it
  items.clear(); stepStart.clear();
  if (lastCtu < 0) lastCtu = wCtu * hCtu - 1;
  int steps = hm355_schedule_step(wCtu, hCtu, wpp, carryLastRow, wCtu - 1, hCtu - 1) + 1;
  const bool tiled = tiles && tiles->count() > 1;
  std::vector<int> tileStep;                 // step of every tile's first CTU
  if (tiled) {
    tileStep.assign(tiles->count(), 0); steps = 0;
    for (int t = 0; t < tiles->count(); t++) {
      const int size = tiles->colWidth[t % tiles->cols] * tiles->rowHeight[t / tiles->cols];
      if (carryTiles && hm355_tile_carries(*tiles, t, width, height)) tileStep[t] = tileStep[t - 1] + tiles->colWidth[(t - 1) % tiles->cols] * tiles->rowHeight[(t - 1) / tiles->cols];
      if (tileStep[t] + size > steps) steps = tileStep[t] + size;
    }
  }
  const bool sliced = !tiled && !wpp && slices && slices->count() > 1;
  std::vector<int> sliceStep, sliceOf;       // step of every slice's first CTU; slice of every CTU
  if (sliced) {
    sliceStep.assign(slices->count(), 0); sliceOf.resize(wCtu * hCtu); steps = 0;
    for (int k = 0; k < slices->count(); k++) {
      const int size = slices->start[k + 1] - slices->start[k];
      if (carryTiles && hm355_slice_carries(*slices, k, wCtu, width, height)) sliceStep[k] = sliceStep[k - 1] + slices->start[k] - slices->start[k - 1];
      if (sliceStep[k] + size > steps) steps = sliceStep[k] + size;
      for (int a = slices->start[k]; a < slices->start[k + 1]; a++) sliceOf[a] = k;
    }
  }
  std::vector<std::vector<WorkItem> > bucket(steps);
  for (int a = firstCtu; a <= lastCtu; a++) {
    const int x = a % wCtu, y = a / wCtu; WorkItem w = {0, x, y, 0};
    int s = hm355_schedule_step(wCtu, hCtu, wpp, carryLastRow, x, y);
    if (tiled) { const int t = tiles->tileOf[a]; s = tileStep[t] + tiles->rsToTs[a] - tiles->rsToTs[tiles->firstCtu[t]]; }
    if (sliced) s = sliceStep[sliceOf[a]] + a - slices->start[sliceOf[a]];
    bucket[s].push_back(w);
  }
  for (int s = 0; s < steps; s++) {
    stepStart.push_back((int)items.size());
    for (int f = 0; f < nFrames; f++) for (size_t i = 0; i < bucket[s].size(); i++) { WorkItem w = bucket[s][i]; w.frame = firstFrame + f; items.push_back(w); }
  }
  stepStart.push_back((int)items.size());
}

// ---- the shape of a search launch (run_begin / lane_init of hm355.hip): pure integer arithmetic, so that tests/hostsim/hostsim_plan.cpp can sweep it ----
// needs HM_CTU_WAVES (hm355_core.h), HM_TEAM and HM_TEAM_I (hm355_team.h): both users include hm355_core.h first
#define HM_WS_MAX 3072   /* 12 searches per CU x 256 CUs is the most that can be resident */
// the widest step of the dependency schedule: as many CTUs of `frames` pictures as can ever be ready at once
// chains: independent CABAC chains per picture without WaveFrontSynchro (the tiles of hm355_set_tiles, the slices of hm355_set_slices)
static inline int hm355_max_items_per_step(int wCtu, int hCtu, int wpp, int frames, int chains = 1)
{
  if (!wpp) return frames * chains;
  int best = 0;
  for (int s = 0; s < wCtu + 2 * (hCtu - 1); s++) { int c = 0; for (int y = 0; y < hCtu; y++) { int x = s - 2 * y; if (x >= 0 && x < wCtu) c++; } if (c > best) best = c; }
  return best * frames;
}
// scratch areas (WorkSpace) of a lane: one per search its grid can hold -- a small batch runs as teams of HM_TEAM wavefronts per CTU; never fewer
// than one workgroup of hm355_ctu_kernel needs (a one-CTU picture with max_batch 1 has 9 team workspaces, and a launch of it that may not use
// teams -- a P / B slice with a fast-decision switch on, HM355_TEAM=0 -- used to get a grid of 0 workgroups)
static inline long long hm355_ws_count(int numCtus, int maxBatch)
{
  long long n = (long long)numCtus * maxBatch * HM_TEAM;
  if (n > HM_WS_MAX) n = HM_WS_MAX;
  if (n < HM_CTU_WAVES) n = HM_CTU_WAVES;
  return n;
}
struct hm355_launch_plan {
  long long wsCount, parallel; int total;   // workspaces of the lane; CTUs the launch can offer at a time (estimate); tickets
  int fewWaves;                             // Params::fewWaves
  int teamWanted, waves, want;              // before the capacity is known: team kernel chosen, wavefronts per team, teams asked for (0: no team)
  int useTeam, teams;                       // the launch: hm355_ctu_team_kernel with `teams` workgroups of `waves` wavefronts ...
  int grid, groups;                         // ... or hm355_ctu_kernel with `groups` workgroups of HM_CTU_WAVES searches (grid = groups * HM_CTU_WAVES)
};
// n pictures of wCtu x hCtu CTUs, CTUs [ctu0, ctu1] of each, on a context created with max_batch and WaveFrontSynchro = wpp.  anyInter: a P / B slice
// among them; fast: esd | cfm << 1 | ecu << 2 | full search << 3; envTeam: HM355_TEAM (-1 unset, 0, 1); envTeamWaves: HM355_TEAM_WAVES (0 unset); laneShare:
// hm355_set_lane_share; teamCap: teams the lane's reconstruction windows exist for (the caller grows them to `want` and plans again).
static inline hm355_launch_plan hm355_plan_launch(int wCtu, int hCtu, int wpp, int maxBatch, int n, int ctu0, int ctu1, int anyInter, int fast,
                                                  int envTeam, int envTeamWaves, int laneShare, long long teamCap, int chains = 1)
{ // chains: tiles or slices per picture (1: neither) -- each is a serial chain of CTUs of its own, so n pictures offer n x chains CTUs at a time
  hm355_launch_plan p; memset(&p, 0, sizeof(p));
  p.wsCount = hm355_ws_count(wCtu * hCtu, maxBatch);
  p.total = n * (ctu1 - ctu0 + 1);
  // A WPP picture offers about 16 CTUs at a time (one when the CABAC state chains through all of them).  A launch that cannot keep ~5
  // one-wavefront searches per CU busy prefers the shortest dependency chain over the fewest instructions (fewWaves); one that cannot
  // even give every CU two searches runs as teams of HM_TEAM wavefronts per CTU (HM355_TEAM=0 / 1 overrides for A/B runs).
  // P / B slices: a team (nine wavefronts, one team per CU) takes a one-stream picture through 3x faster than one wavefront per CTU, and 256 teams together do about half of
  // what 2,816 one-wavefront searches do: measured on 1080p low-delay P streams with WaveFrontSynchro (CTU/s, one wavefront / teams): 32 streams
  // 798 / 1,556, 64: 1,538 / 2,356, 128: 2,862 / 2,944 -- teams up to 96 streams (1,024 when every stream is one serial chain of CTUs).
  p.parallel = (long long)n * (wpp ? 16 : chains);
  p.fewWaves = p.parallel < 1280 ? 1 : 0;
  int useTeam = (anyInter ? (wpp ? n <= 96 : p.parallel <= 1024) : p.parallel <= 512) && p.wsCount >= HM_TEAM;
  if (envTeam == 0) useTeam = 0;
  if (envTeam == 1 && p.wsCount >= HM_TEAM) useTeam = 1;
  // hm355_set_fast_decisions: the team protocol starts sub-CUs and partner candidates speculatively, which is not valid once candidates or
  // sub-CUs may be cut short -- a P / B launch with any of the switches on is searched by one wavefront per CTU, whatever HM355_TEAM says
  // hm355_set_motion_search with fast_search 0 (bit 3 of `fast`): the same.  The protocol's token pass (me_token_prepass) repeats the 2Nx2N integer
  // search only to hand m_integerMv2Nx2N on; the full search neither reads nor writes it, and an exhaustive search run twice for nothing
  // costs more than the team saves.
  if (anyInter && fast) useTeam = 0;
  p.waves = anyInter ? HM_TEAM : HM_TEAM_I;   // P / B slices: every chain of candidates on two or three wavefronts (hm355_team.h)
  if (envTeamWaves == HM_TEAM_I) p.waves = HM_TEAM_I;   // A/B runs (five-wavefront teams on P streams: 1,021 / 1,529 / 1,871 CTU/s in the table above)
  p.teamWanted = useTeam;
  if (useTeam) {
    // as many teams as CTUs can ever be ready at once (the wavefront's widest step), a few more so that a finished team finds the next ticket taken
    const int rows = ctu1 / wCtu - ctu0 / wCtu + 1;
    long long want = (long long)hm355_max_items_per_step(wCtu, rows < hCtu ? rows : hCtu, wpp, n, chains) + 2;
    if (want > p.total) want = p.total; if (want > 512) want = 512; if (want > p.wsCount / p.waves) want = p.wsCount / p.waves;
    p.want = (int)want;
    p.teams = (int)(want < teamCap ? want : teamCap);   // without windows (teamCap 0) the launch runs without teams
  }
  if (useTeam && p.teams > 0) { p.useTeam = 1; p.grid = p.teams; return p; }
  p.teams = 0;
  p.grid = p.total < (int)p.wsCount ? p.total : (int)p.wsCount;
  // A caller that keeps `share` launches in flight (hm355_set_lane_share): each launch only takes its share of the searches the device can hold --
  // a persistent workgroup that waits for a neighbouring CTU keeps its place on the CU, so a launch sized for the whole device would lock the
  // others out until its tickets run out, and the launches would run one after the other
  if (laneShare > 1) { const int cap = HM_WS_MAX * 5 / (4 * laneShare); if (p.grid > cap) p.grid = cap; }
  // workgroups of HM_CTU_WAVES independent searches (wavefronts); a search's workspace is blockIdx * HM_CTU_WAVES + wave < wsCount
  p.groups = (p.grid + HM_CTU_WAVES - 1) / HM_CTU_WAVES;
  if (p.groups > (int)(p.wsCount / HM_CTU_WAVES)) p.groups = (int)(p.wsCount / HM_CTU_WAVES);
  p.grid = p.groups * HM_CTU_WAVES;
  return p;
}
