// hm355 -- gfx950 kernels and the C ABI of include/hm355.h.
//
// One workgroup (one 64-lane wavefront) searches one CTU; a launch carries every CTU of every picture
// in the batch whose dependencies are complete (see hm355_build_schedule).  Launches of consecutive
// steps are ordered by the stream, which is also what makes the neighbours' reconstruction, decision
// arrays and CABAC hand-off visible (kernel boundary == device-scope release/acquire).
//
// There is no CPU path in this library: every entry point needs a working HIP device.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "hm355_core.h"
#include "hm355_dbk.h"
#include "hm355_sao.h"
#include "hm355_bits_kernel.h"
#include "hm355_ingest.h"
#include "hm355_picstat.h"
#include "hm355_host_common.h"
#include "../../include/hm355.h"

// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
// Persistent CTU scheduler.  The work list holds every CTU of every picture of the batch in a dependency-
// respecting (topological) order; a workgroup (one wavefront) repeatedly takes the next ticket, waits until the
// CTUs it depends on have published their results, searches its CTU and publishes.  Because tickets are taken
// in topological order and a workgroup only takes a ticket while it is running, the oldest unfinished ticket
// always has its dependencies satisfied: the grid drains for any grid size and any placement.
//   dependencies of CTU (x,y):  left (x-1,y);  above-right (x+1,y-1) (above at the right picture edge)  [WPP]
//                               previous CTU in raster order (CABAC chain)                               [no WPP]
// Hand-off between workgroups follows the agent-scope release/acquire recipe: all stores of the wave, release
// fence, s_waitcnt, relaxed flag store; consumer: relaxed poll by one lane, acquire fence, plain loads.
#define HM_SPIN_TIMEOUT_TICKS (40ull * 100000000ull)   /* 40 s of the 100 MHz wall clock without ANY CTU of the launch being published: bounds every spin (the oldest unfinished ticket always runs, and one CTU search takes at most a second or two) */
typedef __attribute__((address_space(1))) unsigned int gu32;   // global address space: never a flat access

// lane 0 polls the flag of one dependency (relaxed, agent scope); returns non-zero when the run must be abandoned
__device__ __attribute__((noinline)) int hm355_wait_flag(const unsigned int *flag, unsigned int *abortWord, unsigned int epoch)
{
  int bad = 0;
  if (hm_lane() == 0) {
    const gu32 *f = (const gu32 *)flag; gu32 *ab = (gu32 *)abortWord;
    unsigned long long t0 = wall_clock64();
    unsigned int seen = __hip_atomic_load(ab + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // CTUs the launch has published so far
    while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch) {
      __builtin_amdgcn_s_sleep(32);
      int stop = __hip_atomic_load(ab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
      if (!stop && wall_clock64() - t0 > HM_SPIN_TIMEOUT_TICKS) {
        // a serial CABAC chain (no WPP) legitimately keeps the last ticket holders waiting for minutes: give up only when the
        // whole launch has published nothing for the length of the timeout
        const unsigned int now = __hip_atomic_load(ab + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (now != seen) { seen = now; t0 = wall_clock64(); } else stop = 1;
      }
      if (stop) {
        __hip_atomic_store(ab, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // tell everybody to drain
        bad = 1; break;
      }
    }
  }
  return __shfl(bad, 0, 64);
}

// A workgroup holds HM_CTU_WAVES wavefronts, each an independent CTU search with its own ticket loop, LDS state and HBM workspace; they share
// the read-only tables (LdsTables) and nothing else -- no workgroup barrier after the tables are loaded.  Two such workgroups fit a CU: 12 searches.
extern "C" __global__ void __launch_bounds__(64 * HM_CTU_WAVES, 3) hm355_ctu_kernel(const Params *P, const WorkItem *items, int total, unsigned int *sched, unsigned int epoch)
{
  __shared__ WorkItem curItems[HM_CTU_WAVES];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (wave == 0) load_tables();
  __syncthreads();
  WorkItem &curItem = curItems[wave];
  for (;;) {
    int idx = 0;
    if (hm_lane() == 0) idx = (int)atomicAdd(&sched[0], 1u);
    idx = __shfl(idx, 0, 64);
    if (idx >= total) break;
    if (hm_lane() == 0) curItem = items[idx];
    HM_SYNC();
    const int cx = curItem.ctuX, cy = curItem.ctuY, wCtu = P->wCtu;
    const unsigned int *done = P->frames[curItem.frame].done;
    const int a = cy * wCtu + cx;
    int dep0 = -1, dep1 = -1;
    if (P->wpp) {
      if (cx > 0) dep0 = a - 1;
      if (cy > 0) dep1 = (cy - 1) * wCtu + (cx + 1 < wCtu ? cx + 1 : cx);
    } else if (P->tile) dep0 = P->tile[a].prev;                     // tiles: the CTU before it in its tile, none at the tile's first CTU
    else if (P->slice) dep0 = a > P->slice[a].first ? a - 1 : -1;   // slices: the CTU before it, none at the slice's first CTU
    else if (a > 0) dep0 = a - 1;
    // inter slice: a picture-boundary CTU takes the 2Nx2N integer-MV state of its predecessor in coding order (process_ctu)
    int dep2 = (P->wpp && cx == 0 && cy > 0 && P->frames[curItem.frame].imeta && (63 >= P->width || cy * 64 + 63 >= P->height)) ? a - 1 : -1;
    if (P->tile && dep0 < 0 && P->frames[curItem.frame].imeta && (cx * 64 + 63 >= P->width || cy * 64 + 63 >= P->height)) dep2 = P->tile[a].scanPrev;   // ... the last CTU of the tile before
    if (P->slice && dep0 < 0 && a > 0 && P->frames[curItem.frame].imeta && (cx * 64 + 63 >= P->width || cy * 64 + 63 >= P->height)) dep2 = a - 1;   // ... of the slice before
    int bad = 0;
    if (dep0 >= 0) bad = hm355_wait_flag(done + dep0, sched + 1, epoch);
    if (!bad && dep1 >= 0) bad = hm355_wait_flag(done + dep1, sched + 1, epoch);
    if (!bad && dep2 >= 0) bad = hm355_wait_flag(done + dep2, sched + 1, epoch);
    if (bad) break;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    process_ctu(&g_shs[wave], P, &curItem, (int)blockIdx.x * HM_CTU_WAVES + wave);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (hm_lane() == 0) { __hip_atomic_store((gu32 *)(done + a), epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_fetch_add((gu32 *)(sched + 2), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    HM_SYNC();
  }
}

// The same scheduler with a TEAM of wavefronts per CTU (hm355_team.h): wave 0 takes the tickets, waits for the dependencies and runs the
// reference's recursion; waves 1.. evaluate the unsplit candidates it hands them.  Used for launches that cannot fill the device with
// one-wavefront searches (a few pictures, or pictures whose CABAC state chains through every CTU), where the time of ONE CTU search is
// what the launch takes.
extern "C" __global__ void __launch_bounds__(64 * HM_TEAM, 3) hm355_ctu_team_kernel(const Params *P, const WorkItem *items, int total, unsigned int *sched, unsigned int epoch)
{ // blockDim.x = 64 * HM_TEAM_I (I slices only) or 64 * HM_TEAM; dynamic LDS = HM_TEAM_LDS_BYTES(waves)
  Team *T = HM_TEAM_PTR();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x < HM_TEAM - 1) { T->box[threadIdx.x].reqSeq = 0; T->box[threadIdx.x].doneSeq = 0; }
  if (threadIdx.x == 0) { T->quit = 0; T->dead = 0; T->abortWord = sched + 1; T->waves = (int)(blockDim.x >> 6); }
  if (wave == 0) load_tables();
  __syncthreads();
  if (wave != 0) {
    team_helper(T, wave, wave <= HM_TEAM_HELPERS ? P->teamWin + ((size_t)blockIdx.x * HM_TEAM_HELPERS + (size_t)(wave - 1)) * P->teamWinStride : (Pel *)0);
    return;
  }
  for (;;) {
    int idx = 0;
    if (threadIdx.x == 0) idx = (int)atomicAdd(&sched[0], 1u);
    idx = __shfl(idx, 0, 64);
    if (idx >= total) break;
    if (threadIdx.x == 0) T->item = items[idx];
    HM_SYNC();
    const int cx = T->item.ctuX, cy = T->item.ctuY, wCtu = P->wCtu;
    const unsigned int *done = P->frames[T->item.frame].done;
    const int a = cy * wCtu + cx;
    int dep0 = -1, dep1 = -1;
    if (P->wpp) {
      if (cx > 0) dep0 = a - 1;
      if (cy > 0) dep1 = (cy - 1) * wCtu + (cx + 1 < wCtu ? cx + 1 : cx);
    } else if (P->tile) dep0 = P->tile[a].prev;
    else if (P->slice) dep0 = a > P->slice[a].first ? a - 1 : -1;
    else if (a > 0) dep0 = a - 1;
    int dep2 = (P->wpp && cx == 0 && cy > 0 && P->frames[T->item.frame].imeta && (63 >= P->width || cy * 64 + 63 >= P->height)) ? a - 1 : -1;   // as in hm355_ctu_kernel
    if (P->tile && dep0 < 0 && P->frames[T->item.frame].imeta && (cx * 64 + 63 >= P->width || cy * 64 + 63 >= P->height)) dep2 = P->tile[a].scanPrev;
    if (P->slice && dep0 < 0 && a > 0 && P->frames[T->item.frame].imeta && (cx * 64 + 63 >= P->width || cy * 64 + 63 >= P->height)) dep2 = a - 1;
    int bad = 0;
    if (dep0 >= 0) bad = hm355_wait_flag(done + dep0, sched + 1, epoch);
    if (!bad && dep1 >= 0) bad = hm355_wait_flag(done + dep1, sched + 1, epoch);
    if (!bad && dep2 >= 0) bad = hm355_wait_flag(done + dep2, sched + 1, epoch);
    if (bad) break;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    process_ctu(&T->sh[0], P, &T->item, (int)blockIdx.x * T->waves, T);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    if (threadIdx.x == 0) { __hip_atomic_store((gu32 *)(done + a), epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); __hip_atomic_fetch_add((gu32 *)(sched + 2), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    HM_SYNC();
    if (team_ld(&T->dead)) break;
  }
  HM_TEAM_RELEASE();
  team_st(&T->quit, 1u);
}

// batched distortion primitives: one wavefront per n x n block pair
extern "C" __global__ void __launch_bounds__(64) hm355_dist_kernel(int kind, int n, int bitDepth, int count, const Pel *org, const Pel *cur, uint32_t *out)
{
  for (int b = (int)blockIdx.x; b < count; b += (int)gridDim.x) {
    const Pel *o = org + (size_t)b * n * n, *c = cur + (size_t)b * n * n;
    uint32_t v;
    if (kind == 0) v = dist_sad(o, n, c, n, n, 0, bitDepth);
    else if (kind == 3) v = dist_sad(o, n, c, n, n, 1, bitDepth);
    else if (kind == 1) v = dist_sse(o, n, c, n, n, bitDepth);
    else v = dist_hads(o, n, c, n, n, bitDepth);
    if (hm_lane() == 0) out[b] = v;
  }
}
// batched transforms: LDS-staged, one wavefront per block
extern "C" __global__ void __launch_bounds__(64) hm355_transform_kernel(int inverse, int n, int bitDepth, int useDst, int count, const int32_t *in, int32_t *out)
{
  Shared &sh = g_sh;
  load_tables();
  const int l2 = hm_log2(n);
  for (int b = (int)blockIdx.x; b < count; b += (int)gridDim.x) {
    const int32_t *src = in + (size_t)b * n * n; int32_t *dst = out + (size_t)b * n * n;
    HM_PAR_FOR(i, n * n) sh.bufA[(i >> l2) * HM_TSTRIDE + (i & (n - 1))] = src[i];
    HM_SYNC();
    if (inverse) inv_transform(&sh, n, useDst, bitDepth); else fwd_transform(&sh, n, useDst, bitDepth);
    HM_PAR_FOR(i, n * n) dst[i] = sh.bufA[(i >> l2) * HM_TSTRIDE + (i & (n - 1))];
    HM_SYNC();
  }
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
// Device memory owned by one object: n elements of T, freed in the destructor; moved, never copied.
template <class T> struct DevBuf {
  T *p = nullptr; size_t n = 0;
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { reset(); }
  operator T *() const { return p; }
  void reset() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  hipError_t alloc(size_t count)                       // a new allocation (what was held is freed first)
  {
    reset();
    const hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
  hipError_t ensure(size_t count, bool zero = false)   // allocated on first use (zero: and filled with zeros then, synchronously), kept afterwards
  {
    if (p) return hipSuccess;
    const hipError_t e = alloc(count);
    return e == hipSuccess && zero ? hipMemset(p, 0, count * sizeof(T)) : e;
  }
  hipError_t grow(size_t count) { return count > n ? alloc(count) : hipSuccess; }   // at least count elements; the contents are not kept
};
// Pinned host memory owned by one object (hm355_download's staging), freed in the destructor.
struct PinnedBuf {
  unsigned char *p = nullptr; size_t n = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete; PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() { reset(); }
  void reset() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
  hipError_t grow(size_t bytes)                        // at least `bytes`; the contents are not kept
  {
    if (bytes <= n) return hipSuccess;
    reset();
    const hipError_t e = hipHostMalloc((void **)&p, bytes, hipHostMallocDefault);
    if (e == hipSuccess) n = bytes; else p = nullptr;
    return e;
  }
};
static size_t align256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }   // sub-buffers of one allocation or blob start on 256-byte boundaries

// The device buffers of a reference picture, in the order of its blob (hm355_ref_export): the three border-extended planes, then the motion
// field after TComPic::compressMotion.  ref_buf_bytes gives their sizes.
enum RefBuf { REF_Y, REF_CB, REF_CR, REF_PRED_MODE, REF_MV0, REF_REF_IDX0, REF_MV1, REF_REF_IDX1, REF_NBUF };
struct hm355_ref {       // a finished picture as later pictures reference it (device buffers owned by this object)
  RefPicDev dev = {};
  DevBuf<uint8_t> buf[REF_NBUF];
};
struct Slot {           // one picture resident in HBM
  FrameBuf fb = {};     // device pointers + slice parameters (host copy)
  DevBuf<InterMeta> imeta;   // motion arrays of the slot (allocated on first inter use; kept for the deblocking pass)
  DevBuf<Pel> saoSrc[3]; DevBuf<SaoStat> saoStat; DevBuf<SaoCand> saoCand; DevBuf<SaoBlk> saoCoded, saoRecon;   // SAO working buffers (allocated on first use)
  DevBuf<uint8_t> rawIn, rawOut;   // file frames as they are on disk (ingest / output, allocated on first use)
  DevBuf<uint8_t> bitsRaw, bitsPacked; DevBuf<uint32_t> bitsSizes; DevBuf<CabacW> bitsSync; DevBuf<uint32_t> bitsFlag; DevBuf<InterPic> bitsIp; DevBuf<uint32_t> bitsSlice;   // bitstream pass (allocated on first use)
  // cu_qp_delta (hm355_set_dqp): device state of the picture, allocated on first use; dqpOn: the next searches of the slot run with it
  DevBuf<DqpPic> dDqp; DevBuf<int8_t> dCtuQp; DevBuf<CtuDqp> dDqpOut; DevBuf<uint8_t> dRowFlag; int dqpOn = 0, dqpFlagIn = 0;
  std::vector<int8_t> ctuQp; std::vector<uint8_t> rowFlag; hm355_slice_desc lastSlice = {};
  // LCU-level rate control (hm355_set_ctu_rc): the lambda of every CTU (0: the slice's), the device records built from it, the feedback of the search
  std::vector<double> rcLambda; std::vector<CtuRc> rc; DevBuf<CtuRc> dRc; DevBuf<CtuRcOut> dRcOut;
  // slice-resident search (hm355_slice_begin*, hm355_run_ctus, hm355_slice_end): the slice is open, CTUs searched so far, the first CTU of the last
  // hm355_run_ctus (DqpPic::firstCtu); an inter slice keeps its slice-level parameters and the carried integer MVs until hm355_slice_end
  // rcSearched: the CTUs ctusDone counts were searched with the slot armed (their feedback records are valid)
  int sliceOpen = 0, ctusDone = 0, rcSearched = 0; int32_t firstCtu = 0; DevBuf<InterPic> dIp; DevBuf<MvD> dIntMv;
  int motionSet = 0; uint32_t motionSad = 0, motionSse = 0;   // the open inter slice's m_uiLambdaMotionSAD / SSE (CTUs without a lambda of their own)
};
#define HM_QP_SLICE ((int8_t)-128)   /* Slot::ctuQp of a CTU that hm355_set_ctu_rc has not given a QP: the slice QP */
#define HM_BITS_CAP_PER_CTU 16384u   /* bytes reserved per CTU in the raw substream buffers: above the raw size of a 10-bit 4:2:0 CTU (7.7 KB) */
#define HM_MAX_LANES 4
struct Lane {           // one launch of the search in flight: its own stream, scratch areas, work list and scheduler words (lane_init)
  hipStream_t stream = NULL; hipEvent_t ev0 = NULL, ev1 = NULL;
  DevBuf<Params> dP;    // device copy of the kernel parameters with this lane's scratch areas
  DevBuf<WorkSpace> dWs;   // one scratch area per search the lane's grid can hold
  DevBuf<WorkItem> dItems; // the work list, grown to the longest one so far
  DevBuf<unsigned int> dSched; // [0] ticket, [1] abort, [2] CTUs published by the launch (the spin timeout watches it); lane 0: [8] ticket, [9] abort of the bitstream launch
  std::vector<WorkItem> items; std::vector<int> stepStart; std::vector<FrameBuf> fbs;
  long long key[5] = {}; int keyValid = 0, fewWaves = -1, fast = 0;   // fewWaves, fast: the values dP holds (-1: dP not written yet; fast = esd | cfm << 1 | ecu << 2 | the motion search from bit 3)
  int busy = 0, grid = 0, inFixup = 0, prepared = 0;   // prepared: the launch ran on slots an open slice prepared (hm355_run_ctus)
  DevBuf<Pel> dTeamWin; size_t teamCap = 0;   // team launches (hm355_team.h): the helpers' reconstruction windows, for teamCap teams
  ~Lane() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); if (stream) (void)hipStreamDestroy(stream); }
};
struct hm355_ctx {
  hm355_seq_cfg cfg = {};
  Params hp;            // host copy of the kernel parameters: what lane[0].dP holds
  DevBuf<Tables> dTab;
  DevBuf<FrameBuf> dFrames;
  DevBuf<uint8_t> arena;   // the pictures' planes, decision arrays, coefficients, statistics, CABAC states, done words: one allocation
  DevBuf<unsigned long long> prof;   // diagnostic builds only (HM355_PROFILE, HM355_TRACE): Params::prof
  int teamLdsSet = 0;
  PinnedBuf hStage;     // pinned host staging of hm355_download (one picture's results), allocated on first use
  unsigned int epoch = 0;
  std::vector<Slot> slots;
  Lane lane[HM_MAX_LANES];   // lane 0 is built with the context and serves every blocking entry point; 1.. are built on first use
  double lastKernelMs = 0; int lastLaunches = 0, laneShare = 1;
  hm355_launch_shape lastShape = {};   // hm355_last_launch_shape
  std::string err;
  int numCtus = 0;
  DevBuf<DbkParams> dDbk;      // [max_batch] deblocking parameters of the pictures in the slots
  DevBuf<SaoParams> dSao;      // [max_batch] SAO parameters / results of the pictures in the slots
  DevBuf<BitsParams> dBits;    // [max_batch] bitstream pass parameters / results
  DevBuf<IngestParams> dIngest; // [max_batch] ingest / output parameters
  DevBuf<int32_t> dIntraCost;  // [numCtus] hm355_intra_cost
  DevBuf<PicStatParams> dPicStat; DevBuf<PicStatAcc> dPicAcc;   // [max_batch] picture statistics: parameters / accumulators
  // hm355_set_tiles: the layout in force (tiled: more than one tile), its device tables (Params::tile, Params::tileInfo); tileGen counts the
  // layouts set so far, so that a lane's cached work list and Params are never those of another layout
  hm355_tile_tables tiles; int tiled = 0, tileGen = 0;
  DevBuf<TileCtu> dTile; DevBuf<TileInfo> dTileInfo;
  // hm355_set_slices: the partition in force (sliced: more than one slice) and its device tables (Params::slice, Params::sliceStart); a new
  // partition counts as a new layout (tileGen).  Never together with tiles
  hm355_slice_tables slicesT; int sliced = 0;
  DevBuf<SliceCtu> dSlice; DevBuf<int32_t> dSliceStart;
  std::vector<hm355_slice_bits> sliceBits;   // [slot][slice] of the last hm355_encode_slices_run (hm355_slice_bits_info)
};
static int num_substreams(const hm355_ctx *c) { return c->tiled ? c->tiles.count() : (c->sliced ? c->slicesT.count() : (c->hp.wpp ? c->hp.hCtu : 1)); }
#define HM_NO_SLICES(c, who) do { if ((c)->sliced) return fail((c), HM355_ERR_ARG, who ": not with slices (hm355_set_slices): CTU ranges, CTU rows and the cu_qp_delta predictors follow the coding order of a one-slice picture"); } while (0)
#define HM_NO_TILES(c, who) do { if ((c)->tiled) return fail((c), HM355_ERR_ARG, who ": not with tiles (hm355_set_tiles): CTU ranges, CTU rows and the cu_qp_delta predictors follow the untiled coding order"); } while (0)

#define HM_CHECK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return HM355_ERR_DEVICE; } } while (0)

static int fail(hm355_ctx *c, int code, const char *msg) { if (c) c->err = msg; return code; }
static void next_epoch(hm355_ctx *c) { c->epoch++; if (c->epoch == 0) c->epoch = 1; }   // 0 is what a fresh flag array holds

#ifndef HM355_BUILD_ID
#define HM355_BUILD_ID "unknown"
#endif
extern "C" const char *hm355_build_id(void) { return HM355_BUILD_ID; }
extern "C" const char *hm355_last_error(const hm355_ctx *ctx) { return ctx ? ctx->err.c_str() : "no context"; }

// Lane l of the context: its stream, events, scratch areas, scheduler words and parameter block.  hm355_create builds lane 0 (a blocking stream:
// the entry points that are not searches run on it too; its dP is the context's Params, which every other kernel reads); further lanes are
// built on first use with a non-blocking stream.  dWs is not initialised.
static int lane_init(hm355_ctx *c, int l)
{
  Lane &L = c->lane[l];
  if (L.stream) return HM355_OK;
  HM_CHECK(c, l == 0 ? hipStreamCreate(&L.stream) : hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
  HM_CHECK(c, hipEventCreate(&L.ev0)); HM_CHECK(c, hipEventCreate(&L.ev1));
  // one scratch area per search the persistent grid can hold, or fewer when the batch is small (hm355_ws_count, hm355_host_common.h)
  HM_CHECK(c, L.dWs.alloc((size_t)hm355_ws_count(c->numCtus, c->cfg.max_batch)));
  HM_CHECK(c, L.dSched.ensure(16, true));         // 64 bytes, zeroed by a synchronous hipMemset
  HM_CHECK(c, L.dP.alloc(1));
  return HM355_OK;
}

extern "C" int hm355_create(const hm355_seq_cfg *cfg, hm355_ctx **out)
{
  if (!cfg || !out) return HM355_ERR_ARG;
  *out = NULL;
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7) || (cfg->bit_depth != 8 && cfg->bit_depth != 10) ||
      cfg->ctu_size != 64 || cfg->max_cu_depth != 4 || cfg->tu_log2_max != 5 || cfg->tu_log2_min != 2 || cfg->tu_max_depth_intra != 3 ||
      cfg->max_batch < 1 || (cfg->wavefront_synchro != 0 && cfg->wavefront_synchro != 1))
    return HM355_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return HM355_ERR_NO_DEVICE;
  hm355_ctx *c = new hm355_ctx();
  c->cfg = *cfg;
  Params &P = c->hp; memset(&P, 0, sizeof(P));
  P.width = cfg->width; P.height = cfg->height; P.bitDepth = cfg->bit_depth; P.wpp = cfg->wavefront_synchro;
  P.wCtu = (cfg->width + 63) / 64; P.hCtu = (cfg->height + 63) / 64;
  P.stride[0] = P.wCtu * 64; P.stride[1] = P.stride[2] = P.wCtu * 32;
  P.fullSearch = 0; P.searchRange = 64; P.bipredRange = 4;      // hm355_set_motion_search's defaults: FastSearch 1, SearchRange 64, BipredSearchRange 4
  c->numCtus = P.wCtu * P.hCtu;
  *out = c;   // from here on the caller destroys on failure
  { const int rc = lane_init(c, 0); if (rc != HM355_OK) return rc; }
  Tables *ht = new Tables; hm355_build_tables(ht);
  hipError_t e = c->dTab.alloc(1);
  if (e == hipSuccess) e = hipMemcpy(c->dTab, ht, sizeof(Tables), hipMemcpyHostToDevice);
  delete ht;
  HM_CHECK(c, e);
  HM_CHECK(c, c->dFrames.alloc(cfg->max_batch));
  c->slots.resize(cfg->max_batch);
  { // the pictures' buffers come out of ONE allocation (a batch of thousands of small pictures used to mean tens of thousands of hipMallocs)
    size_t planeBytes[3], off = 0;
    for (int k = 0; k < 3; k++) planeBytes[k] = align256((size_t)P.stride[k] * P.hCtu * (k ? 32 : 64) * sizeof(Pel));
    const size_t metaBytes = align256(sizeof(CtuMeta) * c->numCtus), coefBytes = align256(sizeof(TCoeff) * (size_t)c->numCtus * HM_COEF_CTU);
    const size_t statBytes = align256(sizeof(CtuStat) * c->numCtus), endBytes = align256(sizeof(Cabac) * c->numCtus);
    const size_t doneBytes = align256(sizeof(uint32_t) * c->numCtus);
    const size_t slotBytes = 2 * (planeBytes[0] + planeBytes[1] + planeBytes[2]) + metaBytes + coefBytes + statBytes + endBytes + doneBytes;
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && slotBytes * (size_t)cfg->max_batch > freeB) {
      c->err = "hm355_create: max_batch pictures of this size do not fit the device memory"; return HM355_ERR_NOMEM; }
    HM_CHECK(c, c->arena.alloc(slotBytes * (size_t)cfg->max_batch));
    HM_CHECK(c, hipMemset(c->arena, 0, slotBytes * (size_t)cfg->max_batch));      // planes (padding included) and the done words start at zero
    for (int s = 0; s < cfg->max_batch; s++) {
      FrameBuf &fb = c->slots[s].fb;
      uint8_t *p = c->arena + off;
      for (int k = 0; k < 3; k++) { fb.org[k] = (Pel *)p; p += planeBytes[k]; fb.rec[k] = (Pel *)p; p += planeBytes[k]; }
      fb.meta = (CtuMeta *)p; p += metaBytes; fb.coef = (TCoeff *)p; p += coefBytes; fb.stat = (CtuStat *)p; p += statBytes;
      fb.endState = (Cabac *)p; p += endBytes; fb.done = (uint32_t *)p; p += doneBytes;
      off += slotBytes;
    }
  }
  P.tab = c->dTab; P.ws = c->lane[0].dWs; P.frames = c->dFrames;
#ifdef HM355_PROFILE
  HM_CHECK(c, c->prof.alloc(2 * HM_PROF_N)); HM_CHECK(c, hipMemset(c->prof, 0, 2 * HM_PROF_N * sizeof(unsigned long long)));
  P.prof = c->prof;
#elif defined(HM355_TRACE)
  HM_CHECK(c, c->prof.alloc(1 + 3 * (size_t)HM_TRACE_CAP)); HM_CHECK(c, hipMemset(c->prof, 0, sizeof(unsigned long long)));
  P.prof = c->prof;
#endif
  HM_CHECK(c, hipMemcpy(c->lane[0].dP, &P, sizeof(Params), hipMemcpyHostToDevice));
  c->lane[0].fewWaves = P.fewWaves; c->lane[0].fast = P.bipredRange << 4 | P.searchRange << 12;
  return HM355_OK;
}

extern "C" void hm355_destroy(hm355_ctx *c)
{
  if (!c) return;
  for (int l = 0; l < HM_MAX_LANES; l++) if (c->lane[l].busy) (void)hipStreamSynchronize(c->lane[l].stream);
  delete c;
}

// The visible area of the three planes between a slot's planes (padded to whole CTUs) and host planes of 2-byte samples, row after row:
// asynchronous copies on lane 0's stream (the caller waits), or blocking ones
static hipError_t copy_planes(hm355_ctx *c, Pel *const dev[3], uint16_t *const host[3], hipMemcpyKind kind, bool async)
{
  const Params &P = c->hp;
  const bool up = kind == hipMemcpyHostToDevice;
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; k++) {
    const int w = P.width >> (k ? 1 : 0), h = P.height >> (k ? 1 : 0);
    const size_t devPitch = (size_t)P.stride[k] * sizeof(Pel), hostPitch = (size_t)w * 2;
    void *dst = up ? (void *)dev[k] : (void *)host[k]; const void *src = up ? (const void *)host[k] : (const void *)dev[k];
    const size_t dpitch = up ? devPitch : hostPitch, spitch = up ? hostPitch : devPitch;
    e = async ? hipMemcpy2DAsync(dst, dpitch, src, spitch, hostPitch, h, kind, c->lane[0].stream) : hipMemcpy2D(dst, dpitch, src, spitch, hostPitch, h, kind);
  }
  return e;
}

extern "C" int hm355_upload(hm355_ctx *c, int slot, const hm355_planes *org)
{
  if (!c || !org || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  for (int k = 0; k < 3; k++) if (!org->plane[k]) return fail(c, HM355_ERR_ARG, "null plane");
  HM_CHECK(c, copy_planes(c, c->slots[slot].fb.org, org->plane, hipMemcpyHostToDevice, true));
  HM_CHECK(c, hipStreamSynchronize(c->lane[0].stream));
  c->slots[slot].ctusDone = 0;      // a new picture: nothing of it is searched yet
  return HM355_OK;
}

// cu_qp_delta state of a slot for the search about to be launched (hm355_set_dqp armed it): the quantiser parameters of every QP the CTUs can
// take (they depend on the slice's lambda), the CTUs' QPs, m_bEncodeDQP on entry, the per-row assumptions under WaveFrontSynchro
// and the LCU-level rate control's records (hm355_set_ctu_rc) -- for every CTU when the slot holds an open slice (`resident`), so that hm355_set_ctu_rc
// then only replaces the records it changes
static CtuRc slot_rc_record(const hm355_ctx *c, const Slot &sl, int qp, double lambda)   // lambda 0: the slice's (Slot::lastSlice)
{
  CtuRc r = hm355_ctu_rc_record(c->hp.bitDepth, qp, lambda > 0 ? lambda : sl.lastSlice.lambda, sl.lastSlice.chroma_weight);
  if (!(lambda > 0) && sl.motionSet) { r.lambdaMotionSAD = sl.motionSad; r.lambdaMotionSSE = sl.motionSse; }
  return r;
}
static int dqp_prepare(hm355_ctx *c, int slot, const hm355_slice_desc *sd, hipStream_t stream, int resident)
{
  Slot &sl = c->slots[slot]; const Params &P = c->hp;
  sl.lastSlice = *sd;
  if (!sl.dqpOn) { sl.fb.dqp = NULL; return HM355_OK; }
  HM_CHECK(c, sl.dDqp.ensure(1)); HM_CHECK(c, sl.dCtuQp.ensure(c->numCtus));
  HM_CHECK(c, sl.dDqpOut.ensure(c->numCtus)); HM_CHECK(c, sl.dRowFlag.ensure(P.hCtu)); HM_CHECK(c, sl.dRcOut.ensure(c->numCtus));
  DqpPic *hp = new DqpPic; memset(hp, 0, sizeof(*hp));
  hp->flagIn = sl.dqpFlagIn; hp->sliceQp = sd->qp; hp->ctuQp = sl.dCtuQp; hp->out = sl.dDqpOut; hp->rowFlag = sl.dRowFlag;
  hp->rcOut = sl.dRcOut; hp->firstCtu = 0;
  hm355_fill_qp_tab(hp->tab, P.bitDepth, sd->lambda, sd->chroma_weight);
  std::vector<int8_t> q(c->numCtus, (int8_t)sd->qp);
  if (!sl.ctuQp.empty()) for (int a = 0; a < c->numCtus; a++) if (sl.ctuQp[a] != HM_QP_SLICE) q[a] = sl.ctuQp[a];
  int anyLambda = 0;
  for (size_t a = 0; a < sl.rcLambda.size(); a++) anyLambda |= sl.rcLambda[a] > 0;
  if (resident || anyLambda) {
    if (sl.dRc.ensure(c->numCtus) != hipSuccess) { delete hp; c->err = "hm355: out of device memory for the rate control records"; return HM355_ERR_NOMEM; }
    sl.rc.resize(c->numCtus);
    for (int a = 0; a < c->numCtus; a++)
      sl.rc[a] = slot_rc_record(c, sl, q[a], (size_t)a < sl.rcLambda.size() ? sl.rcLambda[a] : 0.0);
    hp->rc = sl.dRc;
  }
  hipError_t e1 = hipMemcpyAsync(sl.dDqp, hp, sizeof(DqpPic), hipMemcpyHostToDevice, stream);
  if (e1 == hipSuccess && hp->rc) e1 = hipMemcpyAsync(sl.dRc, sl.rc.data(), sizeof(CtuRc) * c->numCtus, hipMemcpyHostToDevice, stream);
  if (e1 == hipSuccess) e1 = hipMemcpyAsync(sl.dCtuQp, q.data(), c->numCtus, hipMemcpyHostToDevice, stream);
  if (e1 == hipSuccess) e1 = hipMemcpyAsync(sl.dRowFlag, sl.rowFlag.data(), P.hCtu, hipMemcpyHostToDevice, stream);
  if (e1 == hipSuccess) e1 = hipStreamSynchronize(stream);
  delete hp;
  HM_CHECK(c, e1);
  sl.fb.dqp = sl.dDqp;
  return HM355_OK;
}

// Enqueues the search over CTUs [ctu0, ctu1] (coding order) of the pictures in slots [slot0, slot0 + n) on lane l and returns; the CTUs before ctu0
// are finished (or imported).  slices NULL: the slots were prepared by hm355_slice_begin* (slice parameters, cu_qp_delta state).  Launches of
// different lanes run concurrently (each on its own stream with its own scratch areas), so the drain of one step overlaps the fill of the next;
// their slot ranges must not overlap.
static int run_begin(hm355_ctx *c, int l, int slot0, int n, const hm355_slice_desc *slices, int ctu0, int ctu1)
{
  const Params &P = c->hp;
  int rc = lane_init(c, l);
  if (rc != HM355_OK) return rc;
  Lane &L = c->lane[l];
  if (L.busy) return fail(c, HM355_ERR_ARG, "hm355_run_begin: the lane still has a launch in flight (hm355_run_wait first)");
  if (c->tiled) {
    if (P.wpp) return fail(c, HM355_ERR_ARG, "hm355: tiles with WaveFrontSynchro are not supported (Main / Main10 refuse the combination)");
    if (ctu0 != 0 || ctu1 != c->numCtus - 1) return fail(c, HM355_ERR_ARG, "hm355: a tiled picture is searched whole (no CTU rows or CTU ranges)");
    for (int f = 0; f < n; f++) if (c->slots[slot0 + f].dqpOn) return fail(c, HM355_ERR_ARG, "hm355: tiles with cu_qp_delta / rate control are not supported (hm355_set_dqp is armed on a slot)");
  }
  if (c->sliced) {
    if (P.wpp) return fail(c, HM355_ERR_ARG, "hm355: slices with WaveFrontSynchro are not built yet");
    if (ctu0 != 0 || ctu1 != c->numCtus - 1) return fail(c, HM355_ERR_ARG, "hm355: a picture of several slices is searched whole (no CTU rows or CTU ranges)");
    for (int f = 0; f < n; f++) if (c->slots[slot0 + f].dqpOn) return fail(c, HM355_ERR_ARG, "hm355: slices with cu_qp_delta / rate control are not supported (hm355_set_dqp is armed on a slot)");
  }
  L.fbs.resize(n);
  for (int f = 0; f < n; f++) {
    if (slices) {
      if (slices[f].slice_type != 2) return fail(c, HM355_ERR_ARG, "only I slices are supported");
      if (slices[f].qp < 0 || slices[f].qp > 51 || !(slices[f].lambda > 0) || !(slices[f].chroma_weight > 0)) return fail(c, HM355_ERR_ARG, "bad slice parameters");
      hm355_fill_slice_params(&c->slots[slot0 + f].fb, P.bitDepth, slices[f].qp, slices[f].lambda, slices[f].chroma_weight);
      { const int rc2 = dqp_prepare(c, slot0 + f, slices + f, L.stream, c->slots[slot0 + f].sliceOpen); if (rc2 != HM355_OK) return rc2; }
    }
    L.fbs[f] = c->slots[slot0 + f].fb;
  }
  HM_CHECK(c, hipMemcpyAsync(c->dFrames + slot0, L.fbs.data(), sizeof(FrameBuf) * n, hipMemcpyHostToDevice, L.stream));
  int carry = 0;
  for (int f = 0; f < n; f++) carry |= c->slots[slot0 + f].fb.imeta != NULL && (P.height & 63) != 0;
  int carryTiles = 0;
  for (int f = 0; f < n; f++) carryTiles |= c->slots[slot0 + f].fb.imeta != NULL;
  const long long key[5] = {slot0, n, carry | carryTiles << 1 | (long long)c->tileGen << 2, ctu0, ctu1};      // the cached work list is reused only for the very same launch shape
  if (!L.keyValid || memcmp(key, L.key, sizeof(key)) != 0) {
    L.keyValid = 0;
    hm355_build_schedule(P.wCtu, P.hCtu, P.wpp, n, L.items, L.stepStart, carry, slot0, ctu0, ctu1, c->tiled ? &c->tiles : NULL, carryTiles, P.width, P.height, c->sliced ? &c->slicesT : NULL);
    HM_CHECK(c, L.dItems.grow(L.items.size()));
    HM_CHECK(c, hipMemcpyAsync(L.dItems, L.items.data(), sizeof(WorkItem) * L.items.size(), hipMemcpyHostToDevice, L.stream));
    memcpy(L.key, key, sizeof(key)); L.keyValid = 1;
  }
  // the launch shape (hm355_plan_launch, hm355_host_common.h: which kernel, how many workgroups, Params::fewWaves)
  int anyInter = 0;
  for (int f = 0; f < n; f++) if (c->slots[slot0 + f].fb.imeta) anyInter = 1;
  // what a lane's Params must follow: the switches, full search (bit 3) and the ranges above it.  The planner sees bits 0..3: to it full search
  // is one more switch that rules teams out (hm355_host_common.h)
  const int fastKey = (P.esd | P.cfm << 1 | P.ecu << 2 | P.fullSearch << 3 | P.bipredRange << 4 | P.searchRange << 12) ^ c->tileGen << 21, fast = fastKey & 15;
  const int chains = c->tiled ? c->tiles.count() : (c->sliced ? c->slicesT.count() : 1);
  int envTeam = -1, envTeamWaves = 0;
  { const char *ev = getenv("HM355_TEAM"); if (ev && (ev[0] == '0' || ev[0] == '1')) envTeam = ev[0] - '0'; }
  { const char *ev = getenv("HM355_TEAM_WAVES"); if (ev) envTeamWaves = atoi(ev); }
  const size_t winSamples = (size_t)65 * P.stride[0] + (size_t)33 * (P.stride[1] + P.stride[2]);
  hm355_launch_plan plan = hm355_plan_launch(P.wCtu, P.hCtu, P.wpp, c->cfg.max_batch, n, ctu0, ctu1, anyInter, fast, envTeam, envTeamWaves, c->laneShare, (long long)L.teamCap, chains);
  if ((size_t)plan.wsCount != L.dWs.n || (size_t)plan.total != L.items.size()) return fail(c, HM355_ERR_DEVICE, "hm355: the launch plan does not match the lane");
  if (plan.teamWanted && (size_t)plan.want > L.teamCap) {   // the windows grow only after the lane's stream is idle; without them the launch runs without teams
    HM_CHECK(c, hipStreamSynchronize(L.stream));
    L.teamCap = 0; L.fewWaves = -1;
    if (L.dTeamWin.alloc((size_t)plan.want * HM_TEAM_HELPERS * winSamples) != hipSuccess) (void)hipGetLastError();
    else L.teamCap = (size_t)plan.want;
    plan = hm355_plan_launch(P.wCtu, P.hCtu, P.wpp, c->cfg.max_batch, n, ctu0, ctu1, anyInter, fast, envTeam, envTeamWaves, c->laneShare, (long long)L.teamCap, chains);
  }
  const int fewWaves = plan.fewWaves, waves = plan.waves;
  if (fewWaves != L.fewWaves || fastKey != L.fast) {
    Params lp = c->hp; lp.ws = L.dWs; lp.fewWaves = fewWaves; lp.teamWin = L.dTeamWin; lp.teamWinStride = winSamples;
    if (l == 0) { c->hp.fewWaves = fewWaves; c->hp.teamWin = L.dTeamWin; c->hp.teamWinStride = winSamples; }
    HM_CHECK(c, hipMemcpyAsync(L.dP, &lp, sizeof(Params), hipMemcpyHostToDevice, L.stream));
    HM_CHECK(c, hipStreamSynchronize(L.stream));      // lp is a local
    L.fewWaves = fewWaves; L.fast = fastKey;
  }
  next_epoch(c);
  HM_CHECK(c, hipMemsetAsync(L.dSched, 0, 32, L.stream));       // ticket = 0, abort = 0, published CTUs = 0 (+ the counters of diagnostic builds)
  if (ctu0 > 0)    // the CTUs before the band are complete: they count as published in this run
    for (int f = 0; f < n; f++) HM_CHECK(c, hipMemsetD32Async((hipDeviceptr_t)c->slots[slot0 + f].fb.done, (int)c->epoch, ctu0, L.stream));
  L.prepared = slices == NULL;
  HM_CHECK(c, hipEventRecord(L.ev0, L.stream));
  const int total = plan.total;
  L.grid = plan.grid;
  if (plan.useTeam) {
    const size_t lds = HM_TEAM_LDS_BYTES(waves);
    if (!c->teamLdsSet) { HM_CHECK(c, hipFuncSetAttribute((const void *)hm355_ctu_team_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)HM_TEAM_LDS_BYTES(HM_TEAM))); c->teamLdsSet = 1; }
    hipLaunchKernelGGL(hm355_ctu_team_kernel, dim3(plan.teams), dim3(64 * waves), lds, L.stream, (const Params *)L.dP, (const WorkItem *)L.dItems, total, L.dSched, c->epoch);
  } else {
    if (plan.groups < 1) return fail(c, HM355_ERR_DEVICE, "hm355: a search launch without a workgroup");
    hipLaunchKernelGGL(hm355_ctu_kernel, dim3(plan.groups), dim3(64 * HM_CTU_WAVES), 0, L.stream, (const Params *)L.dP, (const WorkItem *)L.dItems, total, L.dSched, c->epoch);
  }
  HM_CHECK(c, hipGetLastError());
  if (l == 0 && !L.inFixup) {   // hm355_last_launch_shape: the main launch of the call, not the one-slot launches of dqp_verify_rows
    c->lastShape.kernel = plan.useTeam; c->lastShape.waves = plan.useTeam ? waves : HM_CTU_WAVES; c->lastShape.few_waves = fewWaves;
    c->lastShape.workgroups = plan.useTeam ? plan.teams : plan.groups; c->lastShape.tickets = total;
  }
  HM_CHECK(c, hipEventRecord(L.ev1, L.stream));
  L.busy = 1;
  return HM355_OK;
}
static int run_wait(hm355_ctx *c, int l, double *kernelMs);
// WaveFrontSynchro with cu_qp_delta: TEncCu::m_bEncodeDQP reaches the first CTU of a row from the LAST CTU of the row above (coding order), which the
// wavefront has not searched yet when that row starts.  The launch ran on an assumption per row (Slot::rowFlag, "clear" to begin with: a CTU with
// any coded block leaves it clear); here the assumptions are checked against what the rows above actually left, and from the first row that was
// started on a wrong one the picture is searched again with the corrected value -- rare, and then repeated for the rows below.
// Only rows whose first CTU the launch (CTUs [ctu0, ctu1]) searched with the CTU before it in the same launch are checked, and the search again covers
// that row start .. ctu1: a CTU an earlier hm355_run_ctus finished (its feedback may be with the caller) is never searched again.
static int dqp_verify_rows(hm355_ctx *c, int l, int slot0, int n, int ctu0, int ctu1, int prepared)
{
  const Params &P = c->hp;
  if (!P.wpp || P.wCtu < 1) return HM355_OK;
  for (int f = 0; f < n; f++) {
    Slot &sl = c->slots[slot0 + f];
    if (!sl.dqpOn || !sl.fb.dqp) continue;
    const int firstGuess = prepared ? (sl.firstCtu > ctu0 ? sl.firstCtu : ctu0) + 1 : 1;   // a row start at or after it used Slot::rowFlag
    const int yLo = (firstGuess + P.wCtu - 1) / P.wCtu, yHi = ctu1 / P.wCtu;
    std::vector<CtuDqp> out(c->numCtus);
    for (int y = yLo < 1 ? 1 : yLo; y <= yHi; y++) {
      HM_CHECK(c, hipMemcpy(out.data(), sl.dDqpOut, sizeof(CtuDqp) * c->numCtus, hipMemcpyDeviceToHost));
      int bad = -1;
      for (int yy = y; yy <= yHi; yy++) if (sl.rowFlag[yy] != out[(size_t)yy * P.wCtu - 1].flagOut) { bad = yy; break; }
      if (bad < 0) break;
      sl.rowFlag[bad] = out[(size_t)bad * P.wCtu - 1].flagOut;
      const hm355_slice_desc sd = sl.lastSlice;
      int rc = HM355_OK;
      if (prepared) rc = hipMemcpyAsync(sl.dRowFlag.p + bad, &sl.rowFlag[bad], 1, hipMemcpyHostToDevice, c->lane[l].stream) == hipSuccess ? HM355_OK : fail(c, HM355_ERR_DEVICE, "row flag upload failed");
      if (rc == HM355_OK) rc = run_begin(c, l, slot0 + f, 1, prepared ? NULL : &sd, bad * P.wCtu, ctu1);
      if (rc == HM355_OK) rc = run_wait(c, l, NULL);
      if (rc != HM355_OK) return rc;
      y = bad;
    }
  }
  return HM355_OK;
}
static int run_wait(hm355_ctx *c, int l, double *kernelMs)
{
  Lane &L = c->lane[l];
  if (!L.busy) return fail(c, HM355_ERR_ARG, "hm355_run_wait: no launch in flight on this lane");
  L.busy = 0;
  HM_CHECK(c, hipStreamSynchronize(L.stream));
  float ms = 0; HM_CHECK(c, hipEventElapsedTime(&ms, L.ev0, L.ev1));
  unsigned int sched[2] = {0, 0};
  // on the lane's own stream: a copy on the null stream would wait for the launches of every other lane as well (legacy stream semantics)
  HM_CHECK(c, hipMemcpyAsync(sched, L.dSched, sizeof(sched), hipMemcpyDeviceToHost, L.stream));
  HM_CHECK(c, hipStreamSynchronize(L.stream));
#if defined(HM355_TEAMSTAT)
  { unsigned int ts[8] = {0}; (void)hipMemcpy(ts, L.dSched, sizeof(ts), hipMemcpyDeviceToHost);
    if (ts[3]) fprintf(stderr, "[team] CTUs %u: main wavefront %.1f ms/CTU = 8x8 CUs %.1f + waiting for helpers %.1f + rest; re-searched CUs %u\n",
                       ts[3], ts[4] * 1.28e-3 / ts[3], ts[6] * 1.28e-3 / ts[3], ts[5] * 1.28e-3 / ts[3], ts[7]); }
#endif
  if (sched[1] != 0) return fail(c, HM355_ERR_DEVICE, "scheduler aborted: a dependency wait timed out");
  c->lastKernelMs = ms; c->lastLaunches = 1;
  if (kernelMs) *kernelMs = ms;
  if (L.keyValid && !L.inFixup) {
    const int slot0 = (int)L.key[0], n = (int)L.key[1], ctu1 = (int)L.key[4];
    L.inFixup = 1;
    const int rc = dqp_verify_rows(c, l, slot0, n, (int)L.key[3], ctu1, L.prepared);
    L.inFixup = 0; L.keyValid = 0;          // the fix-up launches reused the lane's work list
    c->lastKernelMs = ms;
    if (rc != HM355_OK) return rc;
    for (int f = 0; f < n; f++) {   // every CTU up to ctu1 is searched (hm355_run_ctus, hm355_ctu_rc_feedback)
      Slot &sl = c->slots[slot0 + f];
      sl.ctusDone = ctu1 + 1; sl.rcSearched = sl.fb.dqp != NULL;
    }
  }
  return HM355_OK;
}
static int run_rows_impl(hm355_ctx *c, int slot0, int n, const hm355_slice_desc *slices, int row0, int row1)
{
  const int rc = run_begin(c, 0, slot0, n, slices, row0 * c->hp.wCtu, (row1 + 1) * c->hp.wCtu - 1);
  return rc != HM355_OK ? rc : run_wait(c, 0, NULL);
}

// Pipelined steps: up to HM355_MAX_LANES launches in flight, each over its own slots (declared in include/hm355.h)
extern "C" int hm355_run_begin(hm355_ctx *c, int lane, int first_slot, int n, const hm355_slice_desc *slices)
{
  if (!c || !slices || lane < 0 || lane >= HM_MAX_LANES || n < 1 || first_slot < 0 || first_slot + n > (int)c->slots.size()) return HM355_ERR_ARG;
  for (int f = 0; f < n; f++) if (c->slots[first_slot + f].fb.imeta) return fail(c, HM355_ERR_ARG, "hm355_run_begin: I slices only");
  for (int l = 0; l < HM_MAX_LANES; l++)
    if (l != lane && c->lane[l].busy && c->lane[l].keyValid && first_slot < (int)(c->lane[l].key[0] + c->lane[l].key[1]) && (int)c->lane[l].key[0] < first_slot + n)
      return fail(c, HM355_ERR_ARG, "hm355_run_begin: the slots overlap a launch in flight on another lane");
  return run_begin(c, lane, first_slot, n, slices, 0, c->numCtus - 1);
}
extern "C" int hm355_set_lane_share(hm355_ctx *c, int launches_in_flight)
{
  if (!c || launches_in_flight < 1 || launches_in_flight > HM_MAX_LANES) return HM355_ERR_ARG;
  c->laneShare = launches_in_flight;
  return HM355_OK;
}
// Sticky state of the context (declared in include/hm355.h): it travels to the device in Params with the next launch of each lane
extern "C" int hm355_set_fast_decisions(hm355_ctx *c, int esd, int cfm, int ecu)
{
  if (!c) return HM355_ERR_ARG;
  if ((esd | cfm | ecu) & ~1) return fail(c, HM355_ERR_ARG, "hm355_set_fast_decisions: every switch is 0 or 1");
  for (size_t s = 0; s < c->slots.size(); s++) if (c->slots[s].sliceOpen) return fail(c, HM355_ERR_ARG, "hm355_set_fast_decisions: a slice is open (hm355_slice_end first)");
  for (int l = 0; l < HM_MAX_LANES; l++) if (c->lane[l].busy) return fail(c, HM355_ERR_ARG, "hm355_set_fast_decisions: a launch is in flight (hm355_run_wait first)");
  c->hp.esd = esd; c->hp.cfm = cfm; c->hp.ecu = ecu;
  return HM355_OK;
}
extern "C" int hm355_set_motion_search(hm355_ctx *c, int fast_search, int search_range, int bipred_search_range)
{
  if (!c) return HM355_ERR_ARG;
  if (fast_search != 0 && fast_search != 1) return fail(c, HM355_ERR_ARG, "hm355_set_motion_search: fast_search is 0 (full search) or 1 (TZ); the selective TZ search (FastSearch=2) is not built");
  if (search_range < 1 || search_range > 256) return fail(c, HM355_ERR_ARG, "hm355_set_motion_search: search_range is 1..256");
  if (bipred_search_range < 1 || bipred_search_range > 16) return fail(c, HM355_ERR_ARG, "hm355_set_motion_search: bipred_search_range is 1..16");
  for (size_t s = 0; s < c->slots.size(); s++) if (c->slots[s].sliceOpen) return fail(c, HM355_ERR_ARG, "hm355_set_motion_search: a slice is open (hm355_slice_end first)");
  for (int l = 0; l < HM_MAX_LANES; l++) if (c->lane[l].busy) return fail(c, HM355_ERR_ARG, "hm355_set_motion_search: a launch is in flight (hm355_run_wait first)");
  c->hp.fullSearch = !fast_search; c->hp.searchRange = search_range; c->hp.bipredRange = bipred_search_range;
  return HM355_OK;
}
// Tiles (declared in include/hm355.h).  The tables go to the device here; every lane takes the new Params with its next launch (the layout's
// generation is part of the key its Params are cached under), lane 0 -- whose Params the loop filters and the bitstream pass read -- at once.
extern "C" int hm355_set_tiles(hm355_ctx *c, int num_cols, const int *col_width_ctus, int num_rows, const int *row_height_ctus, int lf_cross_tile)
{
  if (!c) return HM355_ERR_ARG;
  if (lf_cross_tile != 1) return fail(c, HM355_ERR_ARG, "hm355_set_tiles: lf_cross_tile must be 1 (LFCrossTileBoundaryFlag=0 is not built: the loop filters work across tile edges)");
  for (size_t s = 0; s < c->slots.size(); s++) if (c->slots[s].sliceOpen) return fail(c, HM355_ERR_ARG, "hm355_set_tiles: a slice is open (hm355_slice_end first)");
  for (int l = 0; l < HM_MAX_LANES; l++) if (c->lane[l].busy) return fail(c, HM355_ERR_ARG, "hm355_set_tiles: a launch is in flight (hm355_run_wait first)");
  hm355_tile_tables t;
  const char *why = hm355_build_tiles(c->hp.wCtu, c->hp.hCtu, num_cols, col_width_ctus, num_rows, row_height_ctus, &t);
  if (why) { c->err = std::string("hm355_set_tiles: ") + why; return HM355_ERR_ARG; }
  const int tiled = t.count() > 1;
  if (tiled && c->sliced) return fail(c, HM355_ERR_ARG, "hm355_set_tiles: not with slices in force (hm355_set_slices): several slices in a tiled picture are not built");
  if (tiled && c->hp.wpp) return fail(c, HM355_ERR_ARG, "hm355_set_tiles: tiles with WaveFrontSynchro are not supported (Main / Main10 refuse the combination)");
  if (tiled) for (size_t s = 0; s < c->slots.size(); s++) if (c->slots[s].dqpOn) return fail(c, HM355_ERR_ARG, "hm355_set_tiles: tiles with cu_qp_delta / rate control are not supported (hm355_set_dqp is armed on a slot)");
  DevBuf<TileCtu> dTile; DevBuf<TileInfo> dInfo;
  if (tiled) {
    std::vector<TileInfo> info(t.count());
    for (int k = 0; k < t.count(); k++) { info[k].firstCtu = t.firstCtu[k]; info[k].scanStart = t.rsToTs[t.firstCtu[k]]; }
    HM_CHECK(c, dTile.alloc(t.ctu.size())); HM_CHECK(c, dInfo.alloc(info.size()));
    HM_CHECK(c, hipMemcpy(dTile, t.ctu.data(), sizeof(TileCtu) * t.ctu.size(), hipMemcpyHostToDevice));
    HM_CHECK(c, hipMemcpy(dInfo, info.data(), sizeof(TileInfo) * info.size(), hipMemcpyHostToDevice));
  }
  Params np = c->hp; np.tile = dTile; np.tileInfo = dInfo; np.numTiles = tiled ? t.count() : 0;
  HM_CHECK(c, hipMemcpy(c->lane[0].dP, &np, sizeof(Params), hipMemcpyHostToDevice));    // nothing is in flight: the old tables have no reader left
  c->hp = np; c->tiles = t; c->tiled = tiled; c->tileGen = (c->tileGen + 1) & 1023;
  std::swap(c->dTile.p, dTile.p); std::swap(c->dTile.n, dTile.n); std::swap(c->dTileInfo.p, dInfo.p); std::swap(c->dTileInfo.n, dInfo.n);
  for (int l = 0; l < HM_MAX_LANES; l++) c->lane[l].keyValid = 0;
  return HM355_OK;
}
extern "C" void hm355_uniform_tiles(int w_ctu, int h_ctu, int num_cols, int num_rows, int *col_width_ctus, int *row_height_ctus)
{ hm355_tile_uniform_spacing(w_ctu, h_ctu, num_cols, num_rows, col_width_ctus, row_height_ctus); }
// Slices (declared in include/hm355.h): as hm355_set_tiles -- the tables go to the device here, lane 0's Params at once, the other lanes' with
// their next launch.
extern "C" int hm355_set_slices(hm355_ctx *c, int num_slices, const int *first_ctu, int lf_cross_slice)
{
  if (!c) return HM355_ERR_ARG;
  if (lf_cross_slice != 1) return fail(c, HM355_ERR_ARG, "hm355_set_slices: lf_cross_slice must be 1 (LFCrossSliceBoundaryFlag=0 is not built: the loop filters work across slice edges)");
  for (size_t s = 0; s < c->slots.size(); s++) if (c->slots[s].sliceOpen) return fail(c, HM355_ERR_ARG, "hm355_set_slices: a slice is open (hm355_slice_end first)");
  for (int l = 0; l < HM_MAX_LANES; l++) if (c->lane[l].busy) return fail(c, HM355_ERR_ARG, "hm355_set_slices: a launch is in flight (hm355_run_wait first)");
  hm355_slice_tables t;
  const char *why = hm355_build_slices(c->hp.wCtu, c->hp.hCtu, c->hp.wpp, num_slices, first_ctu, &t);
  if (why) { c->err = std::string("hm355_set_slices: ") + why; return HM355_ERR_ARG; }
  const int sliced = t.count() > 1;
  if (sliced && c->tiled) return fail(c, HM355_ERR_ARG, "hm355_set_slices: not with tiles in force (hm355_set_tiles): several slices in a tiled picture are not built");
  if (sliced && c->hp.wpp) return fail(c, HM355_ERR_ARG, "hm355_set_slices: slices with WaveFrontSynchro are not built yet (the search and the bitstream pass code one substream per slice)");
  if (sliced) for (size_t s = 0; s < c->slots.size(); s++) if (c->slots[s].dqpOn) return fail(c, HM355_ERR_ARG, "hm355_set_slices: slices with cu_qp_delta / rate control are not supported (hm355_set_dqp is armed on a slot)");
  DevBuf<SliceCtu> dSlice; DevBuf<int32_t> dStart;
  if (sliced) {
    HM_CHECK(c, dSlice.alloc(t.ctu.size())); HM_CHECK(c, dStart.alloc(t.start.size()));
    HM_CHECK(c, hipMemcpy(dSlice, t.ctu.data(), sizeof(SliceCtu) * t.ctu.size(), hipMemcpyHostToDevice));
    HM_CHECK(c, hipMemcpy(dStart, t.start.data(), sizeof(int32_t) * t.start.size(), hipMemcpyHostToDevice));
  }
  Params np = c->hp; np.slice = dSlice; np.sliceStart = dStart; np.numSlices = sliced ? t.count() : 0;
  HM_CHECK(c, hipMemcpy(c->lane[0].dP, &np, sizeof(Params), hipMemcpyHostToDevice));    // nothing is in flight: the old tables have no reader left
  c->hp = np; c->slicesT = t; c->sliced = sliced; c->tileGen = (c->tileGen + 1) & 1023;
  std::swap(c->dSlice.p, dSlice.p); std::swap(c->dSlice.n, dSlice.n); std::swap(c->dSliceStart.p, dStart.p); std::swap(c->dSliceStart.n, dStart.n);
  for (int l = 0; l < HM_MAX_LANES; l++) c->lane[l].keyValid = 0;
  c->sliceBits.clear();
  return HM355_OK;
}
extern "C" int hm355_fixed_ctu_slices(int w_ctu, int h_ctu, int wpp, int ctus_per_slice, int *first_ctu_out, int cap)
{ return hm355_slice_fixed_ctus(w_ctu, h_ctu, wpp, ctus_per_slice, first_ctu_out, cap); }
extern "C" int hm355_num_slices(const hm355_ctx *c) { return c ? (c->sliced ? c->slicesT.count() : 1) : HM355_ERR_ARG; }
extern "C" int hm355_run_wait(hm355_ctx *c, int lane, double *kernel_ms)
{
  if (!c || lane < 0 || lane >= HM_MAX_LANES) return HM355_ERR_ARG;
  return run_wait(c, lane, kernel_ms);
}

// A timed group of launches on lane 0's stream: ev0, what `enqueue` puts on the stream (it returns the first error), ev1, one wait.  The time
// and the number of launches are what hm355_last_run_info reports.
template <class F> static int timed_launches(hm355_ctx *c, int launches, F enqueue)
{
  Lane &L = c->lane[0];
  HM_CHECK(c, hipEventRecord(L.ev0, L.stream));
  HM_CHECK(c, enqueue(L.stream));
  HM_CHECK(c, hipEventRecord(L.ev1, L.stream));
  HM_CHECK(c, hipStreamSynchronize(L.stream));
  float ms = 0; HM_CHECK(c, hipEventElapsedTime(&ms, L.ev0, L.ev1));
  c->lastKernelMs = ms; c->lastLaunches = launches;
  return HM355_OK;
}
// The FrameBufs of slots 0..n-1 (fbs, n = fbs.size()) and one parameter block per picture (into dst: [max_batch], allocated on first use) go
// to the device for a pass over the slots; returns once they are there.
template <class T> static int stage_slots(hm355_ctx *c, const std::vector<FrameBuf> &fbs, DevBuf<T> &dst, const std::vector<T> &params)
{
  const hipStream_t s = c->lane[0].stream;
  HM_CHECK(c, dst.ensure(c->slots.size()));
  HM_CHECK(c, hipMemcpyAsync(c->dFrames, fbs.data(), sizeof(FrameBuf) * fbs.size(), hipMemcpyHostToDevice, s));
  HM_CHECK(c, hipMemcpyAsync(dst, params.data(), sizeof(T) * fbs.size(), hipMemcpyHostToDevice, s));
  HM_CHECK(c, hipStreamSynchronize(s));
  return HM355_OK;
}

// ------------------------------------------------------------------------------------------------
// cu_qp_delta: adaptive QP / rate control hooks of compressSlice
// ------------------------------------------------------------------------------------------------
extern "C" int hm355_set_dqp(hm355_ctx *c, int slot, const hm355_dqp_desc *d)
{
  if (!c || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  Slot &sl = c->slots[slot];
  // the open slice's device state (DqpPic, records, row assumptions) was built from the arming at hm355_slice_begin*: it stays until hm355_slice_end
  if (sl.sliceOpen) return fail(c, HM355_ERR_ARG, "hm355_set_dqp: a slice is open on the slot (hm355_slice_end first)");
  sl.rcLambda.clear();
  if (!d || !d->use_dqp) { sl.dqpOn = 0; sl.fb.dqp = NULL; sl.ctuQp.clear(); return HM355_OK; }
  HM_NO_TILES(c, "hm355_set_dqp"); HM_NO_SLICES(c, "hm355_set_dqp");
  const int lo = -6 * (c->hp.bitDepth - 8);
  sl.ctuQp.clear();
  if (d->ctu_qp) {
    for (int a = 0; a < c->numCtus; a++) if (d->ctu_qp[a] < lo || d->ctu_qp[a] > 51) return fail(c, HM355_ERR_ARG, "hm355_set_dqp: CTU QP out of range");
    sl.ctuQp.assign(d->ctu_qp, d->ctu_qp + c->numCtus);
  }
  sl.dqpOn = 1; sl.dqpFlagIn = d->dqp_flag_in != 0;
  sl.rowFlag.assign(c->hp.hCtu, 0);
  return HM355_OK;
}
extern "C" int hm355_get_dqp(hm355_ctx *c, int slot, int8_t *qp_out, int32_t *dqp_flag_out)
{
  if (!c || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  Slot &sl = c->slots[slot];
  if (!sl.dqpOn || !sl.dDqpOut) return fail(c, HM355_ERR_ARG, "hm355_get_dqp: the slot was not searched with cu_qp_delta");
  std::vector<CtuDqp> out(c->numCtus);
  HM_CHECK(c, hipMemcpy(out.data(), sl.dDqpOut, sizeof(CtuDqp) * c->numCtus, hipMemcpyDeviceToHost));
  if (qp_out) for (int a = 0; a < c->numCtus; a++) for (int z = 0; z < 256; z++) qp_out[(size_t)a * 256 + z] = z < out[a].firstZ ? out[a].refQp : out[a].qp;
  if (dqp_flag_out) *dqp_flag_out = out[c->numCtus - 1].flagOut;
  return HM355_OK;
}
extern "C" int hm355_preanalyze(hm355_ctx *c, int slot, uint64_t *sums)
{
  if (!c || !sums || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  DevBuf<unsigned long long> d;
  HM_CHECK(c, hipMemcpy(c->dFrames + slot, &c->slots[slot].fb, sizeof(FrameBuf), hipMemcpyHostToDevice));
  HM_CHECK(c, d.alloc((size_t)8 * c->numCtus));
  const Params *dP = c->lane[0].dP;
  const int rc = timed_launches(c, 1, [&](hipStream_t s) {
    hipLaunchKernelGGL(hm355_preanalyze_kernel, dim3(c->numCtus), dim3(64), 0, s, dP, slot, d.p);
    return hipGetLastError();
  });
  if (rc != HM355_OK) return rc;
  HM_CHECK(c, hipMemcpy(sums, d, sizeof(unsigned long long) * d.n, hipMemcpyDeviceToHost));
  return HM355_OK;
}

// ------------------------------------------------------------------------------------------------
// hm355_inter_slice_desc, shared by hm355_compress_slices_inter and hm355_slice_begin_inter: what both accept, and the slice-level parameters of the
// search they build from it (InterPic; the reference pictures are filled in by each entry, then inter_pic_list1)
// ------------------------------------------------------------------------------------------------
static int inter_desc_check(hm355_ctx *c, const hm355_inter_slice_desc *sd, const char *who)
{
  const int isB = sd->base.slice_type == 0;
  if (sd->base.slice_type != 1 && !isB) return fail(c, HM355_ERR_ARG, (std::string(who) + ": P (1) or B (0) slices").c_str());
  if (sd->num_ref_idx[0] < 1 || sd->num_ref_idx[0] > 16 || (isB ? (sd->num_ref_idx[1] < 1 || sd->num_ref_idx[1] > 16) : sd->num_ref_idx[1] != 0) ||
      sd->max_merge_cand < 1 || sd->max_merge_cand > 5 || (sd->cabac_init_type != 0 && sd->cabac_init_type != 1) ||
      sd->col_ref_idx < 0 || sd->col_ref_idx >= sd->num_ref_idx[(isB && !sd->col_from_l0) ? 1 : 0])
    return fail(c, HM355_ERR_ARG, "bad inter slice parameters");
  return HM355_OK;
}
static void inter_pic_params(const hm355_inter_slice_desc *sd, InterPic *ip)
{
  memset(ip, 0, sizeof(*ip));
  ip->sliceType = sd->base.slice_type; ip->poc = sd->poc; ip->numRefIdx[0] = sd->num_ref_idx[0]; ip->numRefIdx[1] = sd->num_ref_idx[1];
  ip->colFromL0 = sd->col_from_l0; ip->colRefIdx = sd->col_ref_idx; ip->tmvp = sd->tmvp; ip->mvdL1Zero = sd->mvd_l1_zero;
  ip->maxMergeCand = sd->max_merge_cand; ip->checkLDC = sd->check_ldc; ip->cabacInitType = sd->cabac_init_type;
  ip->lambdaMotionSAD = sd->lambda_motion_sad; ip->lambdaMotionSSE = sd->lambda_motion_sse;
}
static void inter_pic_list1(const hm355_inter_slice_desc *sd, InterPic *ip)   // TComSlice::setList1IdxToList0Idx, once ref[][] is filled
{
  for (int i1 = 0; i1 < sd->num_ref_idx[1]; i1++) {
    ip->list1ToList0[i1] = -1;
    for (int i0 = 0; i0 < sd->num_ref_idx[0]; i0++) if (ip->ref[0][i0].poc == ip->ref[1][i1].poc) { ip->list1ToList0[i1] = i0; break; }
  }
}

// ------------------------------------------------------------------------------------------------
// LCU-level rate control (TEncSlice.cpp:766-887): a QP and a lambda per CTU, a slice searched CTU range by CTU range with the rate model's
// feedback in between, and the intra cost the model needs before an I picture (TEncSlice::calCostSliceI)
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(hm355_ctu_rc) == sizeof(CtuRcOut), "hm355_ctu_rc mirrors CtuRcOut");
// lambdas hm355_set_ctu_rc accepts: floor(65536 lambda) must fit the motion lambda's 32 bits and the sign-hiding factor (which divides by lambda)
// its 64; the rate model's lambdas (TEncRateCtrl clips them to [0.1, 10000]) lie far inside
#define HM_RC_LAMBDA_MIN 1e-4
#define HM_RC_LAMBDA_MAX 65535.0
// an open slice was begun on an armed slot, so its device state is complete (hm355_set_dqp is refused while it is open)
static bool open_slice_armed(const hm355_ctx *c, const Slot &sl) { return sl.fb.dqp && sl.rc.size() == (size_t)c->numCtus && sl.dRc && sl.dRcOut; }
extern "C" int hm355_set_ctu_rc(hm355_ctx *c, int slot, int first_ctu, int n, const int8_t *qp, const double *lambda)
{
  if (!c || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  Slot &sl = c->slots[slot];
  if (!sl.dqpOn) return fail(c, HM355_ERR_ARG, "hm355_set_ctu_rc: the slot is not armed with cu_qp_delta (hm355_set_dqp with use_dqp 1 first)");
  if (!qp || n < 1 || first_ctu < 0 || first_ctu + n > c->numCtus) return fail(c, HM355_ERR_ARG, "hm355_set_ctu_rc: bad CTU range (or no QPs)");
  if (sl.sliceOpen && !open_slice_armed(c, sl)) return fail(c, HM355_ERR_ARG, "hm355_set_ctu_rc: the open slice was not begun on an armed slot");
  if (sl.sliceOpen && first_ctu < sl.ctusDone) return fail(c, HM355_ERR_ARG, "hm355_set_ctu_rc: those CTUs of the open slice are searched already");
  const int lo = -6 * (c->hp.bitDepth - 8);
  for (int i = 0; i < n; i++) {
    if (qp[i] < lo || qp[i] > 51) return fail(c, HM355_ERR_ARG, "hm355_set_ctu_rc: CTU QP outside [-QpBDOffset, 51]");
    if (lambda && !(lambda[i] >= HM_RC_LAMBDA_MIN && lambda[i] <= HM_RC_LAMBDA_MAX)) return fail(c, HM355_ERR_ARG, "hm355_set_ctu_rc: a lambda must lie in [1e-4, 65535]");
  }
  if (sl.ctuQp.empty()) sl.ctuQp.assign(c->numCtus, HM_QP_SLICE);
  if (sl.rcLambda.empty()) sl.rcLambda.assign(c->numCtus, 0.0);
  for (int i = 0; i < n; i++) { sl.ctuQp[first_ctu + i] = qp[i]; sl.rcLambda[first_ctu + i] = lambda ? lambda[i] : 0.0; }
  if (!sl.sliceOpen) return HM355_OK;        // the next whole-slice search builds the records (dqp_prepare)
  // an open slice: only the changed records and QPs go to the device, on lane 0's stream (the next hm355_run_ctus is ordered behind them)
  for (int i = 0; i < n; i++) sl.rc[first_ctu + i] = slot_rc_record(c, sl, qp[i], lambda ? lambda[i] : 0.0);
  const hipStream_t s = c->lane[0].stream;
  HM_CHECK(c, hipMemcpyAsync(sl.dRc.p + first_ctu, sl.rc.data() + first_ctu, sizeof(CtuRc) * n, hipMemcpyHostToDevice, s));
  HM_CHECK(c, hipMemcpyAsync(sl.dCtuQp.p + first_ctu, sl.ctuQp.data() + first_ctu, (size_t)n, hipMemcpyHostToDevice, s));
  return HM355_OK;
}

// the slot's slice parameters and cu_qp_delta state, once per slice (hm355_run_ctus then uploads only what changes)
static int slice_open(hm355_ctx *c, int slot, const hm355_slice_desc *sd)
{
  Slot &sl = c->slots[slot];
  hm355_fill_slice_params(&sl.fb, c->hp.bitDepth, sd->qp, sd->lambda, sd->chroma_weight);
  const int rc = dqp_prepare(c, slot, sd, c->lane[0].stream, 1);
  if (rc != HM355_OK) return rc;
  sl.sliceOpen = 1; sl.ctusDone = 0; sl.firstCtu = 0;
  return HM355_OK;
}
static int slice_begin_check(hm355_ctx *c, int slot, const hm355_slice_desc *sd)
{
  if (c->lane[0].busy) return fail(c, HM355_ERR_ARG, "hm355_slice_begin: lane 0 has a launch in flight (hm355_run_wait first)");
  if (!c->slots[slot].dqpOn) return fail(c, HM355_ERR_ARG, "hm355_slice_begin: the slot is not armed with cu_qp_delta (hm355_set_dqp with use_dqp 1 first)");
  if (sd->qp < 0 || sd->qp > 51 || !(sd->lambda > 0) || !(sd->chroma_weight > 0)) return fail(c, HM355_ERR_ARG, "bad slice parameters");
  return HM355_OK;
}
extern "C" int hm355_slice_begin(hm355_ctx *c, int slot, const hm355_slice_desc *sd)
{
  if (!c || !sd || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  HM_NO_TILES(c, "hm355_slice_begin"); HM_NO_SLICES(c, "hm355_slice_begin");
  if (sd->slice_type != 2) return fail(c, HM355_ERR_ARG, "hm355_slice_begin: I slices (P / B: hm355_slice_begin_inter)");
  const int rc = slice_begin_check(c, slot, sd);
  if (rc != HM355_OK) return rc;
  FrameBuf &fb = c->slots[slot].fb; fb.imeta = NULL; fb.ip = NULL; fb.intMv = NULL;
  c->slots[slot].motionSet = 0;
  return slice_open(c, slot, sd);
}
extern "C" int hm355_slice_begin_inter(hm355_ctx *c, int slot, const hm355_inter_slice_desc *sd)
{
  if (!c || !sd || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  HM_NO_TILES(c, "hm355_slice_begin_inter"); HM_NO_SLICES(c, "hm355_slice_begin_inter");
  int rc = inter_desc_check(c, sd, "hm355_slice_begin_inter");
  if (rc != HM355_OK) return rc;
  for (int l = 0; l < 2; l++) for (int i = 0; i < sd->num_ref_idx[l]; i++)
    if (!sd->dev_ref[l][i])
      return fail(c, HM355_ERR_ARG, "hm355_slice_begin_inter: device-resident references only (dev_ref, hm355_ref_from_slot); host hm355_ref_pic pictures go through hm355_compress_slices_inter");
  rc = slice_begin_check(c, slot, &sd->base);
  if (rc != HM355_OK) return rc;
  InterPic hip; inter_pic_params(sd, &hip);
  for (int l = 0; l < 2; l++) for (int i = 0; i < sd->num_ref_idx[l]; i++) hip.ref[l][i] = sd->dev_ref[l][i]->dev;
  inter_pic_list1(sd, &hip);
  Slot &sl = c->slots[slot];
  HM_CHECK(c, sl.dIp.ensure(1)); HM_CHECK(c, sl.imeta.ensure(c->numCtus)); HM_CHECK(c, sl.dIntMv.ensure((size_t)c->numCtus * 32));
  HM_CHECK(c, hipMemcpy(sl.dIp, &hip, sizeof(InterPic), hipMemcpyHostToDevice));
  HM_CHECK(c, hipMemset(sl.imeta, 0, sizeof(InterMeta) * c->numCtus));
  HM_CHECK(c, hipMemset(sl.dIntMv, 0, sizeof(MvD) * sl.dIntMv.n));
  sl.fb.imeta = sl.imeta; sl.fb.ip = sl.dIp; sl.fb.intMv = sl.dIntMv;
  sl.motionSet = 1; sl.motionSad = sd->lambda_motion_sad; sl.motionSse = sd->lambda_motion_sse;
  return slice_open(c, slot, &sd->base);
}
extern "C" int hm355_run_ctus(hm355_ctx *c, int first_slot, int n, int first_ctu, int num_ctus)
{
  if (!c || n < 1 || first_slot < 0 || first_slot + n > (int)c->slots.size()) return HM355_ERR_ARG;
  HM_NO_TILES(c, "hm355_run_ctus"); HM_NO_SLICES(c, "hm355_run_ctus");
  if (num_ctus < 1 || first_ctu < 0 || first_ctu + num_ctus > c->numCtus) return fail(c, HM355_ERR_ARG, "hm355_run_ctus: bad CTU range");
  for (int f = 0; f < n; f++) {
    const Slot &sl = c->slots[first_slot + f];
    if (!sl.sliceOpen) return fail(c, HM355_ERR_ARG, "hm355_run_ctus: no slice is open on the slot (hm355_slice_begin / hm355_slice_begin_inter first)");
    if (!open_slice_armed(c, sl)) return fail(c, HM355_ERR_ARG, "hm355_run_ctus: the open slice was not begun on an armed slot");
    if (sl.ctusDone != first_ctu)
      return fail(c, HM355_ERR_ARG, "hm355_run_ctus: first_ctu must equal the number of CTUs already searched in the slice (coding order: no gap, no repeat)");
  }
  for (int f = 0; f < n; f++) {      // DqpPic::firstCtu: a row start of this range takes the real m_bEncodeDQP of the CTU an earlier call finished
    Slot &sl = c->slots[first_slot + f];
    if (!sl.fb.dqp) continue;
    sl.firstCtu = first_ctu;
    HM_CHECK(c, hipMemcpyAsync((uint8_t *)sl.dDqp.p + offsetof(DqpPic, firstCtu), &sl.firstCtu, sizeof(int32_t), hipMemcpyHostToDevice, c->lane[0].stream));
  }
  int rc = run_begin(c, 0, first_slot, n, NULL, first_ctu, first_ctu + num_ctus - 1);
  if (rc == HM355_OK) rc = run_wait(c, 0, NULL);
  return rc;                                // run_wait counted the CTUs as searched
}
extern "C" int hm355_ctu_rc_feedback(hm355_ctx *c, int slot, int first_ctu, int n, hm355_ctu_rc *out)
{
  if (!c || !out || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  const Slot &sl = c->slots[slot];
  if (!sl.rcSearched || !sl.dRcOut) return fail(c, HM355_ERR_ARG, "hm355_ctu_rc_feedback: the slot's picture was not searched with cu_qp_delta");
  if (n < 1 || first_ctu < 0 || first_ctu + n > sl.ctusDone) return fail(c, HM355_ERR_ARG, "hm355_ctu_rc_feedback: those CTUs are not searched yet");
  HM_CHECK(c, hipMemcpy(out, sl.dRcOut.p + first_ctu, sizeof(CtuRcOut) * n, hipMemcpyDeviceToHost));
  return HM355_OK;
}
extern "C" int hm355_download_inter(hm355_ctx *c, int slot, hm355_ctu_inter_out *ictus)
{
  if (!c || !ictus || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  if (!c->slots[slot].imeta) return fail(c, HM355_ERR_ARG, "hm355_download_inter: the slot holds no motion data");
  HM_CHECK(c, hipMemcpy(ictus, c->slots[slot].imeta, sizeof(InterMeta) * c->numCtus, hipMemcpyDeviceToHost));
  return HM355_OK;
}
extern "C" int hm355_slice_end(hm355_ctx *c, int slot)
{
  if (!c || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  Slot &sl = c->slots[slot];
  if (!sl.sliceOpen) return fail(c, HM355_ERR_ARG, "hm355_slice_end: no slice is open on the slot");
  // the slot as hm355_compress_slices_inter leaves it: the motion arrays stay in Slot::imeta for the loop filter, the bitstream pass and
  // hm355_ref_from_slot; the searches that follow start from the slot's slice parameters again
  sl.sliceOpen = 0; sl.fb.imeta = NULL; sl.fb.ip = NULL; sl.fb.intMv = NULL;
  return HM355_OK;
}
extern "C" int hm355_intra_cost(hm355_ctx *c, int slot, int32_t *cost)
{
  if (!c || !cost || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  HM_CHECK(c, hipMemcpy(c->dFrames + slot, &c->slots[slot].fb, sizeof(FrameBuf), hipMemcpyHostToDevice));
  HM_CHECK(c, c->dIntraCost.ensure(c->numCtus));
  const Params *dP = c->lane[0].dP; int32_t *d = c->dIntraCost;
  const int rc = timed_launches(c, 1, [&](hipStream_t s) {
    hipLaunchKernelGGL(hm355_intra_cost_kernel, dim3(c->numCtus), dim3(64), 0, s, dP, slot, d);
    return hipGetLastError();
  });
  if (rc != HM355_OK) return rc;
  HM_CHECK(c, hipMemcpy(cost, d, sizeof(int32_t) * c->numCtus, hipMemcpyDeviceToHost));
  return HM355_OK;
}

extern "C" int hm355_run(hm355_ctx *c, int n, const hm355_slice_desc *slices)
{
  if (!c || !slices || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  const int rc = run_rows_impl(c, 0, n, slices, 0, c->hp.hCtu - 1);
  return rc;
}

// ------------------------------------------------------------------------------------------------
// CTU-row bands: one device searches rows [first_row, last_row] of its pictures; what the band below needs from the
// band's last row travels through hm355_export_boundary / hm355_import_boundary (host buffers; the transport is the caller's)
// ------------------------------------------------------------------------------------------------
extern "C" int hm355_run_rows(hm355_ctx *c, int first_slot, int n, const hm355_slice_desc *slices, int first_row, int last_row)
{
  if (!c || !slices || n < 1 || first_slot < 0 || first_slot + n > (int)c->slots.size()) return HM355_ERR_ARG;
  HM_NO_TILES(c, "hm355_run_rows"); HM_NO_SLICES(c, "hm355_run_rows");
  if (first_row < 0 || last_row < first_row || last_row >= c->hp.hCtu) return fail(c, HM355_ERR_ARG, "hm355_run_rows: bad row range");
  if (first_row > 0 && !c->hp.wpp) return fail(c, HM355_ERR_ARG, "hm355_run_rows: a band below the first row needs WaveFrontSynchro=1 (without it the CABAC state chains through every CTU)");
  for (int f = 0; f < n; f++) if (c->slots[first_slot + f].fb.imeta) return fail(c, HM355_ERR_ARG, "hm355_run_rows: I slices only");
  return run_rows_impl(c, first_slot, n, slices, first_row, last_row);
}
// bytes of one picture's boundary row: the bottom sample line of the three planes, the decision arrays and the CABAC state after each CTU of the row
extern "C" size_t hm355_boundary_bytes(const hm355_ctx *c)
{
  if (!c) return 0;
  const Params &P = c->hp;
  return (size_t)(P.stride[0] + P.stride[1] + P.stride[2]) * sizeof(Pel) + (size_t)P.wCtu * (sizeof(CtuMeta) + sizeof(Cabac));
}
static int boundary_copy(hm355_ctx *c, int slot, int row, void *buf, int toHost)
{
  if (!c || !buf || slot < 0 || slot >= (int)c->slots.size() || row < 0 || row >= c->hp.hCtu) return HM355_ERR_ARG;
  HM_NO_TILES(c, "hm355_export_boundary / hm355_import_boundary"); HM_NO_SLICES(c, "hm355_export_boundary / hm355_import_boundary");
  const Params &P = c->hp; FrameBuf &fb = c->slots[slot].fb;
  uint8_t *p = (uint8_t *)buf;
  const hipMemcpyKind kind = hipMemcpyDefault;       // buf may be host or device memory (a device buffer goes straight to RCCL)
  for (int k = 0; k < 3; k++) {         // the line right above the next CTU row: all that intra prediction reads across the boundary (TComPattern.cpp:107-165)
    Pel *line = fb.rec[k] + ((size_t)(row + 1) * (k ? 32 : 64) - 1) * P.stride[k];
    const size_t bytes = (size_t)P.stride[k] * sizeof(Pel);
    HM_CHECK(c, toHost ? hipMemcpy(p, line, bytes, kind) : hipMemcpy(line, p, bytes, kind));
    p += bytes;
  }
  CtuMeta *meta = fb.meta + (size_t)row * P.wCtu; Cabac *es = fb.endState + (size_t)row * P.wCtu;
  HM_CHECK(c, toHost ? hipMemcpy(p, meta, sizeof(CtuMeta) * P.wCtu, kind) : hipMemcpy(meta, p, sizeof(CtuMeta) * P.wCtu, kind));
  p += sizeof(CtuMeta) * P.wCtu;
  HM_CHECK(c, toHost ? hipMemcpy(p, es, sizeof(Cabac) * P.wCtu, kind) : hipMemcpy(es, p, sizeof(Cabac) * P.wCtu, kind));
  return HM355_OK;
}
extern "C" int hm355_export_boundary(hm355_ctx *c, int slot, int row, void *buf) { return boundary_copy(c, slot, row, buf, 1); }
extern "C" int hm355_import_boundary(hm355_ctx *c, int slot, int row, const void *buf) { return boundary_copy(c, slot, row, (void *)buf, 0); }

#if defined(HM355_TRACE)
// diagnostic build only: copies and resets the RD-evaluation trace (3 words per record), returns the record count
extern "C" long long hm355_read_trace(hm355_ctx *c, unsigned long long *out, long long cap)
{
  unsigned long long n = 0;
  if (hipMemcpy(&n, c->hp.prof, sizeof(n), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (n > HM_TRACE_CAP) n = HM_TRACE_CAP;
  if ((long long)n > cap) n = (unsigned long long)cap;
  if (n && hipMemcpy(out, c->hp.prof + 1, n * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  hipMemset(c->hp.prof, 0, sizeof(unsigned long long));
  return (long long)n;
}
#endif
#ifdef HM355_PROFILE
extern "C" int hm355_reset_profile(hm355_ctx *c) { return hipMemset(c->hp.prof, 0, 2 * HM_PROF_N * sizeof(unsigned long long)) == hipSuccess ? 0 : HM355_ERR_DEVICE; }
extern "C" int hm355_read_profile(hm355_ctx *c, unsigned long long *out32)
{ return hipMemcpy(out32, c->hp.prof, 2 * HM_PROF_N * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : HM355_ERR_DEVICE; }
#endif

extern "C" int hm355_last_run_info(const hm355_ctx *c, double *kernel_ms, int *launches)
{
  if (!c) return HM355_ERR_ARG;
  if (kernel_ms) *kernel_ms = c->lastKernelMs;
  if (launches) *launches = c->lastLaunches;
  return HM355_OK;
}
extern "C" int hm355_last_launch_shape(const hm355_ctx *c, hm355_launch_shape *out)
{
  if (!c || !out) return HM355_ERR_ARG;
  *out = c->lastShape;
  return HM355_OK;
}

// One CTU as the C ABI carries it (hm355_ctu_out) and as the device holds it (CtuStat, CtuMeta and HM_COEF_CTU coefficients: Y at 0, Cb at
// 4096, Cr at 5120)
static void ctu_to_out(const CtuStat &st, const CtuMeta &m, const TCoeff *cf, hm355_ctu_out *o)
{
  o->total_cost = st.cost; o->total_bits = st.bits; o->total_dist = st.dist;
  memcpy(o->depth, m.depth, 256); memcpy(o->part_size, m.part, 256); memcpy(o->pred_mode, m.pred, 256);
  memcpy(o->intra_dir_luma, m.dirL, 256); memcpy(o->intra_dir_chroma, m.dirC, 256); memcpy(o->tr_idx, m.tr, 256);
  memcpy(o->cbf, m.cbf, 768); memcpy(o->tskip, m.ts, 768);
  memcpy(o->coeff_y, cf, 4096 * 4); memcpy(o->coeff_cb, cf + 4096, 1024 * 4); memcpy(o->coeff_cr, cf + 5120, 1024 * 4);
}
static void ctu_from_out(const hm355_ctu_out &o, CtuMeta *m, TCoeff *cf)   // cf NULL: the CU / TU data only
{
  memcpy(m->depth, o.depth, 256); memcpy(m->part, o.part_size, 256); memcpy(m->pred, o.pred_mode, 256);
  memcpy(m->dirL, o.intra_dir_luma, 256); memcpy(m->dirC, o.intra_dir_chroma, 256); memcpy(m->tr, o.tr_idx, 256);
  memcpy(m->cbf, o.cbf, 768); memcpy(m->ts, o.tskip, 768);
  if (cf) { memcpy(cf, o.coeff_y, 4096 * 4); memcpy(cf + 4096, o.coeff_cb, 1024 * 4); memcpy(cf + 5120, o.coeff_cr, 1024 * 4); }
}

extern "C" int hm355_download(hm355_ctx *c, int slot, hm355_planes *rec, hm355_ctu_out *ctus, hm355_slice_stats *stats)
{
  if (!c || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  const Params &P = c->hp; FrameBuf &fb = c->slots[slot].fb; const hipStream_t s = c->lane[0].stream;
  if (rec) for (int k = 0; k < 3; k++) if (!rec->plane[k]) return fail(c, HM355_ERR_ARG, "null plane");
  // one picture's results cross PCIe into a pinned staging buffer (asynchronous copies on the context's stream, one wait), then go to the caller's
  // pageable buffers with plain memcpy: 81 MB per 4K picture
  const size_t nC = (size_t)c->numCtus, bStat = sizeof(CtuStat) * nC, bMeta = sizeof(CtuMeta) * nC, bCoef = sizeof(TCoeff) * nC * HM_COEF_CTU;
  size_t bPlane[3], oPlane[3], off = align256(bStat + bMeta + bCoef);
  for (int k = 0; k < 3; k++) { bPlane[k] = (size_t)(P.width >> (k ? 1 : 0)) * 2 * (size_t)(P.height >> (k ? 1 : 0)); oPlane[k] = off; off += align256(bPlane[k]); }
  HM_CHECK(c, c->hStage.grow(off));
  unsigned char *hs = c->hStage.p;
  CtuStat *st = (CtuStat *)hs; CtuMeta *meta = (CtuMeta *)(hs + bStat); TCoeff *coef = (TCoeff *)(hs + bStat + bMeta);
  uint16_t *const stagedPlanes[3] = { (uint16_t *)(hs + oPlane[0]), (uint16_t *)(hs + oPlane[1]), (uint16_t *)(hs + oPlane[2]) };
  if (rec) HM_CHECK(c, copy_planes(c, fb.rec, stagedPlanes, hipMemcpyDeviceToHost, true));
  if (ctus || stats) HM_CHECK(c, hipMemcpyAsync(st, fb.stat, bStat, hipMemcpyDeviceToHost, s));
  if (ctus) {
    HM_CHECK(c, hipMemcpyAsync(meta, fb.meta, bMeta, hipMemcpyDeviceToHost, s));
    HM_CHECK(c, hipMemcpyAsync(coef, fb.coef, bCoef, hipMemcpyDeviceToHost, s));
  }
  HM_CHECK(c, hipStreamSynchronize(s));
  if (rec) for (int k = 0; k < 3; k++) memcpy(rec->plane[k], stagedPlanes[k], bPlane[k]);
  if (stats) {
    stats->pic_total_bits = 0; stats->pic_rd_cost = 0; stats->pic_dist = 0;
    for (int a = 0; a < c->numCtus; a++) { stats->pic_total_bits += st[a].bits; stats->pic_rd_cost += st[a].cost; stats->pic_dist += st[a].dist; }
  }
  if (ctus) for (int a = 0; a < c->numCtus; a++) ctu_to_out(st[a], meta[a], coef + (size_t)a * HM_COEF_CTU, ctus + a);
  return HM355_OK;
}

extern "C" int hm355_compress_slices(hm355_ctx *c, int n, const hm355_slice_desc *slices, const hm355_planes *org,
                                     hm355_planes *rec, hm355_ctu_out *const *ctus, hm355_slice_stats *stats)
{
  if (!c || !slices || !org || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  int rc;
  for (int f = 0; f < n; f++) if ((rc = hm355_upload(c, f, org + f)) != HM355_OK) return rc;
  if ((rc = hm355_run(c, n, slices)) != HM355_OK) return rc;
  for (int f = 0; f < n; f++)
    if ((rc = hm355_download(c, f, rec ? rec + f : NULL, ctus ? ctus[f] : NULL, stats ? stats + f : NULL)) != HM355_OK) return rc;
  return HM355_OK;
}

extern "C" int hm355_compress_slice(hm355_ctx *c, const hm355_slice_desc *slice, const hm355_planes *org,
                                    hm355_planes *rec, hm355_ctu_out *ctus, hm355_slice_stats *stats)
{
  hm355_ctu_out *cl[1] = { ctus };
  return hm355_compress_slices(c, 1, slice, org, rec, ctus ? cl : NULL, stats);
}

// ------------------------------------------------------------------------------------------------
// P and B slices: reference pictures are uploaded per call (border-extended like TComPicYuv::extendPicBorder); the n pictures
// of one call are independent of each other (e.g. the current pictures of n streams) and run concurrently
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(hm355_ctu_inter_out) == sizeof(InterMeta), "hm355_ctu_inter_out mirrors InterMeta");
static void ref_buf_bytes(const hm355_ctx *c, size_t bytes[REF_NBUF])
{
  const size_t np = (size_t)c->numCtus * 256;
  for (int k = 0; k < 3; k++) {
    const int cw = c->hp.width >> (k ? 1 : 0), ch = c->hp.height >> (k ? 1 : 0), mg = HM_REF_MARGIN >> (k ? 1 : 0);
    bytes[REF_Y + k] = (size_t)(cw + 2 * mg) * (ch + 2 * mg) * sizeof(Pel);
  }
  bytes[REF_PRED_MODE] = np; bytes[REF_MV0] = bytes[REF_MV1] = np * sizeof(MvD); bytes[REF_REF_IDX0] = bytes[REF_REF_IDX1] = np;
}
// allocates the buffers of r (ref_buf_bytes) and points r->dev at them
static hipError_t ref_alloc(hm355_ctx *c, hm355_ref *r)
{
  size_t bytes[REF_NBUF]; ref_buf_bytes(c, bytes);
  for (int i = 0; i < REF_NBUF; i++) { const hipError_t e = r->buf[i].alloc(bytes[i]); if (e != hipSuccess) return e; }
  for (int k = 0; k < 3; k++) {
    const int mg = HM_REF_MARGIN >> (k ? 1 : 0), st = (c->hp.width >> (k ? 1 : 0)) + 2 * mg;
    r->dev.plane[k] = (const Pel *)r->buf[REF_Y + k].p + (size_t)mg * st + mg; r->dev.stride[k] = st;
  }
  r->dev.predMode = r->buf[REF_PRED_MODE];
  r->dev.mv[0] = (const MvD *)r->buf[REF_MV0].p; r->dev.refIdx[0] = (const int8_t *)r->buf[REF_REF_IDX0].p;
  r->dev.mv[1] = (const MvD *)r->buf[REF_MV1].p; r->dev.refIdx[1] = (const int8_t *)r->buf[REF_REF_IDX1].p;
  return hipSuccess;
}
static hipError_t upload_ref_pic(hm355_ctx *c, const hm355_ref_pic *hp, hm355_ref *r)
{
  const Params &P = c->hp;
  size_t bytes[REF_NBUF]; ref_buf_bytes(c, bytes);
  hipError_t e = ref_alloc(c, r);
  for (int cc = 0; cc < 3 && e == hipSuccess; cc++) {
    const int cw = P.width >> (cc ? 1 : 0), ch = P.height >> (cc ? 1 : 0), mg = HM_REF_MARGIN >> (cc ? 1 : 0), st = r->dev.stride[cc];
    std::vector<Pel> buf(bytes[REF_Y + cc] / sizeof(Pel));
    for (int y = -mg; y < ch + mg; y++) {
      const int sy = y < 0 ? 0 : (y >= ch ? ch - 1 : y);
      Pel *d = buf.data() + (size_t)(y + mg) * st + mg;
      const uint16_t *srow = hp->plane[cc] + (size_t)sy * cw;
      for (int x = 0; x < cw; x++) d[x] = (Pel)srow[x];
      for (int x = 1; x <= mg; x++) { d[-x] = (Pel)srow[0]; d[cw - 1 + x] = (Pel)srow[cw - 1]; }
    }
    e = hipMemcpy(r->buf[REF_Y + cc], buf.data(), bytes[REF_Y + cc], hipMemcpyHostToDevice);
  }
  const void *motion[REF_NBUF - REF_PRED_MODE] = { hp->pred_mode, hp->mv[0], hp->ref_idx[0], hp->mv[1], hp->ref_idx[1] };
  for (int i = REF_PRED_MODE; i < REF_NBUF && e == hipSuccess; i++) e = hipMemcpy(r->buf[i], motion[i - REF_PRED_MODE], bytes[i], hipMemcpyHostToDevice);
  for (int l = 0; l < 2; l++) { memcpy(r->dev.refPoc[l], hp->ref_poc[l], sizeof(r->dev.refPoc[l])); memcpy(r->dev.refLT[l], hp->ref_lt[l], sizeof(r->dev.refLT[l])); }
  r->dev.poc = hp->poc; r->dev.isLongTerm = hp->long_term;
  return e;
}
extern "C" int hm355_compress_slices_inter(hm355_ctx *c, int n, const hm355_inter_slice_desc *slices, const hm355_planes *org,
                                           hm355_planes *rec, hm355_ctu_out *const *ctus, hm355_ctu_inter_out *const *ictus, hm355_slice_stats *stats)
{
  if (!c || !slices || !org || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  for (int f = 0; f < n; f++) {
    const hm355_inter_slice_desc *sd = slices + f;
    const int rc0 = inter_desc_check(c, sd, "hm355_compress_slices_inter");
    if (rc0 != HM355_OK) return rc0;
    for (int l = 0; l < 2; l++) for (int i = 0; i < sd->num_ref_idx[l]; i++) {
      const hm355_ref_pic *hp = sd->ref[l][i];
      if (sd->dev_ref[l][i]) continue;
      if (!hp || !hp->plane[0] || !hp->plane[1] || !hp->plane[2] || !hp->pred_mode || !hp->mv[0] || !hp->mv[1] || !hp->ref_idx[0] || !hp->ref_idx[1])
        return fail(c, HM355_ERR_ARG, "null reference picture data");
    }
  }
  int rc;
  for (int f = 0; f < n; f++) if ((rc = hm355_upload(c, f, org + f)) != HM355_OK) return rc;
  std::vector<const hm355_ref_pic *> seen; std::vector<hm355_ref> uploaded;     // a picture referenced several times is uploaded once
  std::vector<DevBuf<InterPic>> dIp(n); std::vector<DevBuf<MvD>> dIntMv(n);
  std::vector<hm355_slice_desc> base(n);
  hipError_t e = hipSuccess;
  for (int f = 0; f < n && e == hipSuccess; f++) {
    const hm355_inter_slice_desc *sd = slices + f;
    InterPic hip; inter_pic_params(sd, &hip);
    for (int l = 0; l < 2; l++) for (int i = 0; i < sd->num_ref_idx[l] && e == hipSuccess; i++) {
      if (sd->dev_ref[l][i]) { hip.ref[l][i] = sd->dev_ref[l][i]->dev; continue; }
      const hm355_ref_pic *hp = sd->ref[l][i];
      size_t k = 0; for (; k < seen.size(); k++) if (seen[k] == hp) break;
      if (k == seen.size()) { uploaded.emplace_back(); e = upload_ref_pic(c, hp, &uploaded.back()); seen.push_back(hp); }
      hip.ref[l][i] = uploaded[k].dev;
    }
    inter_pic_list1(sd, &hip);
    Slot &sl = c->slots[f];
    sl.motionSet = 1; sl.motionSad = sd->lambda_motion_sad; sl.motionSse = sd->lambda_motion_sse;   // CTUs without a lambda of their own (hm355_set_ctu_rc)
    if (e == hipSuccess) e = dIp[f].alloc(1);
    if (e == hipSuccess) e = hipMemcpy(dIp[f], &hip, sizeof(InterPic), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = sl.imeta.ensure(c->numCtus);
    if (e == hipSuccess) e = hipMemset(sl.imeta, 0, sizeof(InterMeta) * c->numCtus);
    if (e == hipSuccess) e = dIntMv[f].alloc((size_t)c->numCtus * 32);
    if (e == hipSuccess) e = hipMemset(dIntMv[f], 0, sizeof(MvD) * dIntMv[f].n);
    sl.fb.imeta = sl.imeta; sl.fb.ip = dIp[f]; sl.fb.intMv = dIntMv[f];
    base[f] = sd->base; base[f].slice_type = 2;            // hm355_run validates the common fields
  }
  if (e != hipSuccess) { c->err = std::string("reference picture upload: ") + hipGetErrorString(e); rc = HM355_ERR_DEVICE; }
  else rc = hm355_run(c, n, base.data());
  for (int f = 0; f < n && rc == HM355_OK; f++) {
    rc = hm355_download(c, f, rec ? rec + f : NULL, ctus ? ctus[f] : NULL, stats ? stats + f : NULL);
    if (rc == HM355_OK && ictus && ictus[f] && hipMemcpy(ictus[f], c->slots[f].imeta, sizeof(InterMeta) * c->numCtus, hipMemcpyDeviceToHost) != hipSuccess) { c->err = "motion download failed"; rc = HM355_ERR_DEVICE; }
  }
  for (int f = 0; f < n; f++) { FrameBuf &fb = c->slots[f].fb; fb.imeta = NULL; fb.ip = NULL; fb.intMv = NULL; }
  return rc;
}
extern "C" int hm355_compress_slice_inter(hm355_ctx *c, const hm355_inter_slice_desc *sd, const hm355_planes *org,
                                          hm355_planes *rec, hm355_ctu_out *ctus, hm355_ctu_inter_out *ictus, hm355_slice_stats *stats)
{
  hm355_ctu_out *cl[1] = { ctus }; hm355_ctu_inter_out *il[1] = { ictus };
  return hm355_compress_slices_inter(c, 1, sd, org, rec, ctus ? cl : NULL, ictus ? il : NULL, stats);
}

// ------------------------------------------------------------------------------------------------
// device-resident reference pictures
// ------------------------------------------------------------------------------------------------
extern "C" void hm355_ref_release(hm355_ctx *c, hm355_ref *r)
{
  (void)c;
  delete r;
}
extern "C" int hm355_ref_from_slot(hm355_ctx *c, int slot, int32_t poc, int32_t is_inter, const int32_t num_ref[2], const int32_t ref_poc[2][16],
                                   const int32_t ref_lt[2][16], hm355_ref **out)
{
  if (!c || !out || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  if (is_inter && !c->slots[slot].imeta) return fail(c, HM355_ERR_ARG, "hm355_ref_from_slot: the slot holds no motion data");
  const Params &P = c->hp; const hipStream_t s = c->lane[0].stream; const Params *dP = c->lane[0].dP;
  std::unique_ptr<hm355_ref> r(new hm355_ref());
  FrameBuf fbh = c->slots[slot].fb; fbh.imeta = is_inter ? c->slots[slot].imeta.p : NULL;
  hipError_t e = hipMemcpy(c->dFrames + slot, &fbh, sizeof(FrameBuf), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = ref_alloc(c, r.get());
  if (e == hipSuccess) {
    uint8_t *pm = r->buf[REF_PRED_MODE]; MvD *mv0 = (MvD *)r->buf[REF_MV0].p, *mv1 = (MvD *)r->buf[REF_MV1].p;
    int8_t *ri0 = (int8_t *)r->buf[REF_REF_IDX0].p, *ri1 = (int8_t *)r->buf[REF_REF_IDX1].p;
    for (int k = 0; k < 3; k++) {
      const int ch = P.height >> (k ? 1 : 0), mg = HM_REF_MARGIN >> (k ? 1 : 0), st = r->dev.stride[k];
      hipLaunchKernelGGL(hm355_ref_kernel, dim3((st + 63) / 64, ch + 2 * mg, 1), dim3(64, 1, 1), 0, s, dP, slot, k, (Pel *)r->buf[REF_Y + k].p, pm, mv0, mv1, ri0, ri1);
    }
    const size_t np = (size_t)c->numCtus * 256;
    hipLaunchKernelGGL(hm355_ref_kernel, dim3((unsigned)((np + 63) / 64), 1, 1), dim3(64, 1, 1), 0, s, dP, slot, 3, (Pel *)r->buf[REF_Y].p, pm, mv0, mv1, ri0, ri1);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) { c->err = std::string("hm355_ref_from_slot: ") + hipGetErrorString(e); return HM355_ERR_DEVICE; }
  r->dev.poc = poc; r->dev.isLongTerm = 0;
  if (ref_poc) memcpy(r->dev.refPoc, ref_poc, sizeof(r->dev.refPoc));
  if (ref_lt) memcpy(r->dev.refLT, ref_lt, sizeof(r->dev.refLT));
  (void)num_ref;
  *out = r.release();
  return HM355_OK;
}

// A finished reference picture as one blob ("Inter (C5)": pictures of one temporal layer run on different devices, the finished
// pictures are all-gathered): header, the three border-extended planes, the compressed motion field.  buf may be host or device memory,
// so a device buffer goes to RCCL as it is.
struct RefBlobHdr { uint32_t magic, width, height, bitDepth; int32_t stride[3], poc, isLongTerm, refPoc[2][16], refLT[2][16]; double user[4]; };
extern "C" size_t hm355_ref_bytes(const hm355_ctx *c)
{
  if (!c) return 0;
  size_t bytes[REF_NBUF]; ref_buf_bytes(c, bytes);
  size_t n = align256(sizeof(RefBlobHdr));
  for (int i = 0; i < REF_NBUF; i++) n += align256(bytes[i]);
  return n;
}
static int ref_blob_copy(hm355_ctx *c, hm355_ref *r, uint8_t *p, int toBlob)
{ // the buffers of r in the order of RefBuf, each at a 256-byte boundary of the blob
  size_t bytes[REF_NBUF]; ref_buf_bytes(c, bytes);
  for (int i = 0; i < REF_NBUF; i++) if (!r->buf[i]) return fail(c, HM355_ERR_ARG, "hm355_ref_export / import: not a device-resident reference picture");
  for (int i = 0; i < REF_NBUF; i++) {
    HM_CHECK(c, toBlob ? hipMemcpy(p, r->buf[i], bytes[i], hipMemcpyDefault) : hipMemcpy(r->buf[i], p, bytes[i], hipMemcpyDefault));
    p += align256(bytes[i]);
  }
  return HM355_OK;
}
extern "C" int hm355_ref_export(hm355_ctx *c, const hm355_ref *r, void *buf, const double user[4])
{
  if (!c || !r || !buf) return HM355_ERR_ARG;
  RefBlobHdr h; memset(&h, 0, sizeof(h));
  h.magic = 0x52464d48u; h.width = (uint32_t)c->hp.width; h.height = (uint32_t)c->hp.height; h.bitDepth = (uint32_t)c->hp.bitDepth;
  for (int k = 0; k < 3; k++) h.stride[k] = r->dev.stride[k];
  h.poc = r->dev.poc; h.isLongTerm = r->dev.isLongTerm; memcpy(h.refPoc, r->dev.refPoc, sizeof(h.refPoc)); memcpy(h.refLT, r->dev.refLT, sizeof(h.refLT));
  if (user) memcpy(h.user, user, sizeof(h.user));
  HM_CHECK(c, hipMemcpy(buf, &h, sizeof(h), hipMemcpyDefault));
  return ref_blob_copy(c, (hm355_ref *)r, (uint8_t *)buf + align256(sizeof(RefBlobHdr)), 1);
}
extern "C" int hm355_ref_import(hm355_ctx *c, const void *buf, hm355_ref **out, double user[4])
{
  if (!c || !buf || !out) return HM355_ERR_ARG;
  RefBlobHdr h;
  HM_CHECK(c, hipMemcpy(&h, buf, sizeof(h), hipMemcpyDefault));
  if (h.magic != 0x52464d48u || (int)h.width != c->hp.width || (int)h.height != c->hp.height || (int)h.bitDepth != c->hp.bitDepth)
    return fail(c, HM355_ERR_ARG, "hm355_ref_import: not a reference picture of this sequence");
  std::unique_ptr<hm355_ref> r(new hm355_ref());
  if (ref_alloc(c, r.get()) != hipSuccess) { (void)hipGetLastError(); return fail(c, HM355_ERR_NOMEM, "hm355_ref_import: out of device memory"); }
  for (int k = 0; k < 3; k++) if (h.stride[k] != r->dev.stride[k]) return fail(c, HM355_ERR_ARG, "hm355_ref_import: plane layout mismatch");
  r->dev.poc = h.poc; r->dev.isLongTerm = h.isLongTerm; memcpy(r->dev.refPoc, h.refPoc, sizeof(h.refPoc)); memcpy(r->dev.refLT, h.refLT, sizeof(h.refLT));
  if (user) memcpy(user, h.user, sizeof(h.user));
  const int rc = ref_blob_copy(c, r.get(), (uint8_t *)buf + align256(sizeof(RefBlobHdr)), 0);
  if (rc != HM355_OK) return rc;
  *out = r.release();
  return HM355_OK;
}

// ------------------------------------------------------------------------------------------------
// deblocking (TComLoopFilter::loopFilterPic): in place on the reconstruction planes of the slots
// ------------------------------------------------------------------------------------------------
extern "C" int hm355_deblock_run(hm355_ctx *c, int n, const hm355_dbk_desc *descs)
{
  if (!c || !descs || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  const Params &P = c->hp;
  std::vector<FrameBuf> fbs(n); std::vector<DbkParams> dps(n);
  for (int f = 0; f < n; f++) {
    if (descs[f].slice_type < 0 || descs[f].slice_type > 2 || descs[f].qp < 0 || descs[f].qp > 51) return fail(c, HM355_ERR_ARG, "bad deblocking parameters");
    if (descs[f].slice_type != 2 && !c->slots[f].imeta) return fail(c, HM355_ERR_ARG, "hm355_deblock_run: the slot holds no motion data (run hm355_compress_slices_inter first)");
    fbs[f] = c->slots[f].fb; fbs[f].imeta = descs[f].slice_type != 2 ? c->slots[f].imeta.p : NULL;
    dps[f].sliceType = descs[f].slice_type; dps[f].qp = descs[f].qp; memcpy(dps[f].refPoc, descs[f].ref_poc, sizeof(dps[f].refPoc));
  }
  const int rc = stage_slots(c, fbs, c->dDbk, dps);
  if (rc != HM355_OK) return rc;
  const int w = P.width, h = P.height;
  const dim3 blk(64, 1, 1);
  const Params *dP = c->lane[0].dP; const DbkParams *dDbk = c->dDbk;
  return timed_launches(c, 4, [&](hipStream_t s) {
    // vertical edges (luma, chroma), then horizontal edges: the stream orders the two directions
    hipLaunchKernelGGL(hm355_dbk_kernel, dim3((w / 8 + 63) / 64, h / 4, n), blk, 0, s, dP, dDbk, 0);
    hipLaunchKernelGGL(hm355_dbk_kernel, dim3((w / 16 + 63) / 64, h / 4, n), blk, 0, s, dP, dDbk, 1);
    hipLaunchKernelGGL(hm355_dbk_kernel, dim3((w / 4 + 63) / 64, (h / 8 > 1 ? h / 8 : 1), n), blk, 0, s, dP, dDbk, 2);
    hipLaunchKernelGGL(hm355_dbk_kernel, dim3((w / 4 + 63) / 64, (h / 16 > 1 ? h / 16 : 1), n), blk, 0, s, dP, dDbk, 3);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------------------------------------------
// sample adaptive offset (TEncSampleAdaptiveOffset::SAOProcess) on the deblocked pictures of the slots
// ------------------------------------------------------------------------------------------------
extern "C" int hm355_sao_run(hm355_ctx *c, int n, hm355_sao_desc *descs)
{
  if (!c || !descs || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  const Params &P = c->hp;
  std::vector<FrameBuf> fbs(n); std::vector<SaoParams> sps(n);
  for (int f = 0; f < n; f++) {
    hm355_sao_desc &d = descs[f];
    if (d.qp < 0 || d.qp > 51 || d.cabac_init_type < 0 || d.cabac_init_type > 2 || d.depth < 0 || d.depth > 7 || !(d.lambda > 0) || !(d.chroma_weight > 0))
      return fail(c, HM355_ERR_ARG, "bad SAO parameters");
    Slot &sl = c->slots[f];
    for (int k = 0; k < 3; k++) HM_CHECK(c, sl.saoSrc[k].ensure((size_t)P.stride[k] * P.hCtu * (k ? 32 : 64)));
    HM_CHECK(c, sl.saoStat.ensure(3 * (size_t)c->numCtus));
    HM_CHECK(c, sl.saoCand.ensure(3 * SAO_NUM_TYPES * (size_t)c->numCtus));
    HM_CHECK(c, sl.saoCoded.ensure(c->numCtus));
    HM_CHECK(c, sl.saoRecon.ensure(c->numCtus));
    fbs[f] = sl.fb;
    SaoParams &sp = sps[f]; memset(&sp, 0, sizeof(sp));
    sp.qp = d.qp; sp.cabacInitType = d.cabac_init_type; sp.depth = d.depth;
    sp.lambda[0] = d.lambda; sp.lambda[1] = sp.lambda[2] = d.lambda / d.chroma_weight;
    for (int k = 0; k < 3; k++) { sp.disabledPrev[k] = d.depth > 0 ? d.disabled_rate[k][d.depth - 1] : 0.0; sp.src[k] = sl.saoSrc[k]; }
    sp.stat = sl.saoStat; sp.cand = sl.saoCand; sp.coded = sl.saoCoded; sp.recon = sl.saoRecon;
    for (int k = 0; k < 3; k++) HM_CHECK(c, hipMemcpyAsync(sl.saoSrc[k], sl.fb.rec[k], sizeof(Pel) * sl.saoSrc[k].n, hipMemcpyDeviceToDevice, c->lane[0].stream));
  }
  int rc = stage_slots(c, fbs, c->dSao, sps);
  if (rc != HM355_OK) return rc;
  const Params *dP = c->lane[0].dP; SaoParams *dSao = c->dSao;
  rc = timed_launches(c, 3, [&](hipStream_t s) {
    hipLaunchKernelGGL(hm355_sao_stats_kernel, dim3(c->numCtus, 3, n), dim3(64, 1, 1), 0, s, dP, dSao);
    hipLaunchKernelGGL(hm355_sao_decide_kernel, dim3(n, 1, 1), dim3(64, 1, 1), 0, s, dP, dSao);
    hipLaunchKernelGGL(hm355_sao_apply_kernel, dim3((P.width + 63) / 64, P.height, 3 * n), dim3(64, 1, 1), 0, s, dP, dSao);
    return hipGetLastError();
  });
  if (rc != HM355_OK) return rc;
  HM_CHECK(c, hipMemcpy(sps.data(), c->dSao, sizeof(SaoParams) * n, hipMemcpyDeviceToHost));
  for (int f = 0; f < n; f++) {
    hm355_sao_desc &d = descs[f];
    for (int k = 0; k < 3; k++) { d.enabled[k] = sps[f].enabled[k]; d.disabled_rate[k][d.depth] = (double)sps[f].numOff[k] / (double)c->numCtus; }
    if (d.params) {
      std::vector<SaoBlk> blk(c->numCtus);
      HM_CHECK(c, hipMemcpy(blk.data(), c->slots[f].saoCoded, sizeof(SaoBlk) * c->numCtus, hipMemcpyDeviceToHost));
      static_assert(sizeof(SaoBlk) == 3 * 35 * 4, "SaoBlk is 3 x (mode, type, aux, offset[32])");
      memcpy(d.params, blk.data(), sizeof(SaoBlk) * c->numCtus);
    }
  }
  return HM355_OK;
}

// host buffers in and out: rec is filtered in place with the CU / TU / motion data of the same slice
extern "C" int hm355_deblock(hm355_ctx *c, const hm355_dbk_desc *desc, const hm355_ctu_out *ctus, const hm355_ctu_inter_out *ictus, hm355_planes *rec)
{
  if (!c || !desc || !ctus || !rec) return HM355_ERR_ARG;
  if (desc->slice_type != 2 && !ictus) return fail(c, HM355_ERR_ARG, "hm355_deblock: inter slices need the motion data");
  Slot &sl = c->slots[0]; FrameBuf &fb = sl.fb;
  for (int k = 0; k < 3; k++) if (!rec->plane[k]) return fail(c, HM355_ERR_ARG, "null plane");
  HM_CHECK(c, copy_planes(c, fb.rec, rec->plane, hipMemcpyHostToDevice, false));
  std::vector<CtuMeta> meta(c->numCtus);
  for (int a = 0; a < c->numCtus; a++) ctu_from_out(ctus[a], &meta[a], NULL);
  HM_CHECK(c, hipMemcpy(fb.meta, meta.data(), sizeof(CtuMeta) * c->numCtus, hipMemcpyHostToDevice));
  if (desc->slice_type != 2) {
    HM_CHECK(c, sl.imeta.ensure(c->numCtus));
    HM_CHECK(c, hipMemcpy(sl.imeta, ictus, sizeof(InterMeta) * c->numCtus, hipMemcpyHostToDevice));
  }
  int rc = hm355_deblock_run(c, 1, desc);
  if (rc != HM355_OK) return rc;
  HM_CHECK(c, copy_planes(c, fb.rec, rec->plane, hipMemcpyDeviceToHost, false));
  return HM355_OK;
}

// ------------------------------------------------------------------------------------------------
// picture ingest / output (TVideoIOYuv::read / ::write) between file frames and the slots
// ------------------------------------------------------------------------------------------------
static int ingest_launch(hm355_ctx *c, int n, const std::vector<IngestParams> &ips, int output, int gridW, int gridH)
{
  std::vector<FrameBuf> fbs(n); for (int f = 0; f < n; f++) fbs[f] = c->slots[f].fb;
  const int rc = stage_slots(c, fbs, c->dIngest, ips);
  if (rc != HM355_OK) return rc;
  const dim3 grid(((unsigned)((gridW + 7) / 8) * (unsigned)gridH + HM_INGEST_BLOCK - 1) / HM_INGEST_BLOCK, 1, 3 * n);   // sized for the luma plane
  const Params *dP = c->lane[0].dP; const IngestParams *dIngest = c->dIngest;
  return timed_launches(c, 1, [&](hipStream_t s) {
    if (output) hipLaunchKernelGGL(hm355_output_kernel, grid, dim3(HM_INGEST_BLOCK), 0, s, dP, dIngest);
    else hipLaunchKernelGGL(hm355_ingest_kernel, grid, dim3(HM_INGEST_BLOCK), 0, s, dP, dIngest);
    return hipGetLastError();
  });
}

extern "C" int hm355_upload_file_frames(hm355_ctx *c, int n, const void *const *frames, int file_width, int file_height, int file_bit_depth)
{
  if (!c || !frames || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  const Params &P = c->hp;
  if (file_width < 2 || file_height < 2 || (file_width & 1) || (file_height & 1) || file_width > P.width || file_height > P.height ||
      file_bit_depth < 8 || file_bit_depth > 14) return fail(c, HM355_ERR_ARG, "hm355_upload_file_frames: bad file frame geometry / bit depth");
  const size_t maxBytes = (size_t)P.width * P.height * 3, bytes = (size_t)file_width * file_height * 3 / 2 * (file_bit_depth > 8 ? 2 : 1);
  std::vector<IngestParams> ips(n);
  for (int f = 0; f < n; f++) {
    if (!frames[f]) return fail(c, HM355_ERR_ARG, "null frame");
    Slot &sl = c->slots[f];
    HM_CHECK(c, sl.rawIn.ensure(maxBytes));
    HM_CHECK(c, hipMemcpyAsync(sl.rawIn, frames[f], bytes, hipMemcpyHostToDevice, c->lane[0].stream));
    sl.ctusDone = 0;
    ips[f].src = sl.rawIn; ips[f].dst = NULL; ips[f].fileW = file_width; ips[f].fileH = file_height; ips[f].fileBitDepth = file_bit_depth; ips[f].fromOrg = 0;
  }
  return ingest_launch(c, n, ips, 0, P.width, P.height);
}

extern "C" int hm355_download_org(hm355_ctx *c, int slot, hm355_planes *org)
{
  if (!c || !org || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  for (int k = 0; k < 3; k++) if (!org->plane[k]) return fail(c, HM355_ERR_ARG, "null plane");
  HM_CHECK(c, copy_planes(c, c->slots[slot].fb.org, org->plane, hipMemcpyDeviceToHost, false));
  return HM355_OK;
}

extern "C" int hm355_download_file_frames(hm355_ctx *c, int n, void *const *frames, int file_bit_depth, int conf_right, int conf_bottom, int source)
{
  if (!c || !frames || n < 1 || n > (int)c->slots.size() || source < 0 || source > 1) return HM355_ERR_ARG;
  const Params &P = c->hp;
  if (conf_right < 0 || conf_bottom < 0 || (conf_right & 1) || (conf_bottom & 1) || conf_right >= P.width || conf_bottom >= P.height ||
      file_bit_depth < 8 || file_bit_depth > 14) return fail(c, HM355_ERR_ARG, "hm355_download_file_frames: bad conformance window / bit depth");
  const int fw = P.width - conf_right, fh = P.height - conf_bottom;
  const size_t maxBytes = (size_t)P.width * P.height * 3, bytes = (size_t)fw * fh * 3 / 2 * (file_bit_depth > 8 ? 2 : 1);
  std::vector<IngestParams> ips(n);
  for (int f = 0; f < n; f++) {
    if (!frames[f]) return fail(c, HM355_ERR_ARG, "null frame");
    Slot &sl = c->slots[f];
    HM_CHECK(c, sl.rawOut.ensure(maxBytes));
    ips[f].src = NULL; ips[f].dst = sl.rawOut; ips[f].fileW = fw; ips[f].fileH = fh; ips[f].fileBitDepth = file_bit_depth; ips[f].fromOrg = source;
  }
  int rc = ingest_launch(c, n, ips, 1, fw, fh);
  if (rc != HM355_OK) return rc;
  for (int f = 0; f < n; f++) HM_CHECK(c, hipMemcpy(frames[f], c->slots[f].rawOut, bytes, hipMemcpyDeviceToHost));
  return HM355_OK;
}

// ------------------------------------------------------------------------------------------------
// picture statistics (TEncGOP::xCalculateAddPSNR, the decoded picture hash) on the pictures of the slots
// ------------------------------------------------------------------------------------------------
extern "C" int hm355_picture_stats_run(hm355_ctx *c, int n, hm355_picstat_desc *descs)
{
  if (!c || !descs || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  const Params &P = c->hp;
  std::vector<FrameBuf> fbs(n); std::vector<PicStatParams> pps(n);
  int anyCrc = 0, anyMd5 = 0;
  for (int f = 0; f < n; f++) {
    const hm355_picstat_desc &d = descs[f];
    if (d.hash_method < 0 || d.hash_method > 3) return fail(c, HM355_ERR_ARG, "hm355_picture_stats_run: hash_method must be 0 (none), 1 (MD5), 2 (CRC) or 3 (checksum)");
    if (d.pad_right < 0 || d.pad_bottom < 0 || (d.pad_right & 1) || (d.pad_bottom & 1) || d.pad_right >= P.width || d.pad_bottom >= P.height)
      return fail(c, HM355_ERR_ARG, "hm355_picture_stats_run: the pads must be even, not negative and smaller than the picture");
    fbs[f] = c->slots[f].fb;
    pps[f].hashMethod = d.hash_method; pps[f].padRight = d.pad_right; pps[f].padBottom = d.pad_bottom; pps[f].pad = 0;
    anyMd5 |= d.hash_method == 1; anyCrc |= d.hash_method == 2;
  }
  HM_CHECK(c, c->dPicAcc.ensure(c->slots.size()));
  int rc = stage_slots(c, fbs, c->dPicStat, pps);
  if (rc != HM355_OK) return rc;
  const Params *dP = c->lane[0].dP; const PicStatParams *dPp = c->dPicStat; PicStatAcc *dAcc = c->dPicAcc;
  const int groups = ((P.width + 7) / 8) * P.height, chunks = ps_crc_chunks_per_row(P.width, HM_CRC_CHUNK) * P.height;
  rc = timed_launches(c, 1 + anyCrc + anyMd5, [&](hipStream_t s) {
    const hipError_t e = hipMemsetAsync(dAcc, 0, sizeof(PicStatAcc) * n, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hm355_picstat_kernel, dim3((groups + HM_PS_BLOCK * HM_PS_GROUPS - 1) / (HM_PS_BLOCK * HM_PS_GROUPS), 1, 3 * n), dim3(HM_PS_BLOCK), 0, s, dP, dPp, dAcc);
    if (anyCrc) hipLaunchKernelGGL(hm355_crc_kernel, dim3((chunks + HM_PS_BLOCK - 1) / HM_PS_BLOCK, 1, 3 * n), dim3(HM_PS_BLOCK), 0, s, dP, dPp, dAcc, HM_CRC_CHUNK);
    if (anyMd5) hipLaunchKernelGGL(hm355_md5_kernel, dim3((n + 63) / 64, 3, 1), dim3(64), 0, s, dP, dPp, dAcc, n);
    return hipGetLastError();
  });
  if (rc != HM355_OK) return rc;
  std::vector<PicStatAcc> acc(n);
  HM_CHECK(c, hipMemcpy(acc.data(), c->dPicAcc, sizeof(PicStatAcc) * n, hipMemcpyDeviceToHost));
  const int bps = P.bitDepth > 8 ? 2 : 1;
  for (int f = 0; f < n; f++) {
    hm355_picstat_desc &d = descs[f];
    memset(d.digest, 0, sizeof(d.digest));
    d.digest_len = d.hash_method == 1 ? 16 : (d.hash_method == 2 ? 2 : (d.hash_method == 3 ? 4 : 0));
    for (int k = 0; k < 3; k++) {
      const int cs = k ? 1 : 0, wc = P.width >> cs, hc = P.height >> cs;
      const int size = (wc - (d.pad_right >> cs)) * (hc - (d.pad_bottom >> cs));
      d.ssd[k] = acc[f].ssd[k];
      d.psnr[k] = ps_psnr(acc[f].ssd[k], size, P.bitDepth);       // the reference's expressions and libm call
      d.mse[k] = ps_mse(acc[f].ssd[k], size);
      if (d.hash_method == 1) for (int i = 0; i < 16; i++) d.digest[k][i] = (uint8_t)(acc[f].md5[k][i >> 2] >> (8 * (i & 3)));
      else if (d.hash_method == 2) { const uint32_t v = acc[f].crc[k] ^ ps_crc_init_term(wc, hc, bps); d.digest[k][0] = (uint8_t)(v >> 8); d.digest[k][1] = (uint8_t)v; }
      else if (d.hash_method == 3) for (int i = 0; i < 4; i++) d.digest[k][i] = (uint8_t)(acc[f].cksum[k] >> (24 - 8 * i));
    }
  }
  return HM355_OK;
}

extern "C" int hm355_upload_rec(hm355_ctx *c, int slot, const hm355_planes *rec)
{
  if (!c || !rec || slot < 0 || slot >= (int)c->slots.size()) return HM355_ERR_ARG;
  for (int k = 0; k < 3; k++) if (!rec->plane[k]) return fail(c, HM355_ERR_ARG, "null plane");
  HM_CHECK(c, copy_planes(c, c->slots[slot].fb.rec, rec->plane, hipMemcpyHostToDevice, false));
  return HM355_OK;
}

// host buffers in: the two pictures go to slot 0 first
extern "C" int hm355_picture_stats(hm355_ctx *c, hm355_picstat_desc *desc, const hm355_planes *org, const hm355_planes *rec)
{
  if (!c || !desc || !org || !rec) return HM355_ERR_ARG;
  for (int k = 0; k < 3; k++) if (!org->plane[k] || !rec->plane[k]) return fail(c, HM355_ERR_ARG, "null plane");
  Slot &sl = c->slots[0];
  HM_CHECK(c, copy_planes(c, sl.fb.org, org->plane, hipMemcpyHostToDevice, false));
  HM_CHECK(c, copy_planes(c, sl.fb.rec, rec->plane, hipMemcpyHostToDevice, false));
  sl.ctusDone = 0;                  // a new picture
  return hm355_picture_stats_run(c, 1, desc);
}

// ------------------------------------------------------------------------------------------------
// bitstream pass (TEncSlice::encodeSlice) on the pictures of the slots
// ------------------------------------------------------------------------------------------------
extern "C" int hm355_num_substreams(const hm355_ctx *c) { return c ? num_substreams(c) : HM355_ERR_ARG; }

extern "C" int hm355_encode_slices_run(hm355_ctx *c, int n, hm355_bits_desc *descs)
{
  if (!c || !descs || n < 1 || n > (int)c->slots.size()) return HM355_ERR_ARG;
  const Params &P = c->hp; Lane &L0 = c->lane[0];
  const int numSub = num_substreams(c), subCap = numSub > P.hCtu ? numSub : P.hCtu;
  c->sliceBits.clear();                          // hm355_slice_bits_info has nothing to return unless this call succeeds
  const size_t rawBytes = (size_t)c->numCtus * HM_BITS_CAP_PER_CTU;
  std::vector<FrameBuf> fbs(n); std::vector<BitsParams> bps(n);
  next_epoch(c);
  for (int f = 0; f < n; f++) {
    hm355_bits_desc &d = descs[f];
    if (d.slice_type < 0 || d.slice_type > 2 || d.qp < 0 || d.qp > 51 || !d.out || !d.sub_sizes) return fail(c, HM355_ERR_ARG, "bad bitstream pass parameters");
    Slot &sl = c->slots[f];
    if (d.slice_type != 2) {
      if (!sl.imeta) return fail(c, HM355_ERR_ARG, "hm355_encode_slices_run: the slot holds no motion data (run hm355_compress_slices_inter first)");
      if (d.cabac_init_type < 0 || d.cabac_init_type > 1 || d.num_ref_idx[0] < 1 || d.num_ref_idx[0] > 16 || d.num_ref_idx[1] < 0 || d.num_ref_idx[1] > 16 ||
          d.max_merge_cand < 1 || d.max_merge_cand > 5) return fail(c, HM355_ERR_ARG, "bad inter slice header values");
    }
    if ((d.sao_enabled[0] || d.sao_enabled[1]) && !sl.saoCoded) return fail(c, HM355_ERR_ARG, "hm355_encode_slices_run: the slot holds no SAO parameters (run hm355_sao_run first)");
    HM_CHECK(c, sl.bitsRaw.ensure(rawBytes)); HM_CHECK(c, sl.bitsPacked.ensure(rawBytes));
    HM_CHECK(c, sl.bitsSizes.grow(subCap)); HM_CHECK(c, sl.bitsSync.ensure(P.hCtu));
    HM_CHECK(c, sl.bitsFlag.ensure(P.hCtu, true));
    if (c->sliced) HM_CHECK(c, sl.bitsSlice.grow((size_t)3 * numSub));      // per slice: the table it chose, its bins, the flag that publishes both
    fbs[f] = sl.fb; fbs[f].imeta = NULL; fbs[f].ip = NULL;
    if (d.slice_type != 2) {
      HM_CHECK(c, sl.bitsIp.ensure(1));
      std::vector<InterPic> ipv(1); InterPic &ip = ipv[0];   // only the slice header values the PU syntax reads
      memset(&ip, 0, sizeof(ip));
      ip.sliceType = d.slice_type; ip.numRefIdx[0] = d.num_ref_idx[0]; ip.numRefIdx[1] = d.slice_type == 0 ? d.num_ref_idx[1] : 0;
      ip.mvdL1Zero = d.mvd_l1_zero; ip.maxMergeCand = d.max_merge_cand; ip.cabacInitType = d.cabac_init_type;
      HM_CHECK(c, hipMemcpy(sl.bitsIp, &ip, sizeof(InterPic), hipMemcpyHostToDevice));
      fbs[f].imeta = sl.imeta; fbs[f].ip = sl.bitsIp;
    }
    BitsParams &bp = bps[f]; memset(&bp, 0, sizeof(bp));
    bp.sliceType = d.slice_type; bp.qp = d.qp; bp.cabacInitType = d.cabac_init_type;
    bp.saoEnabled[0] = d.sao_enabled[0]; bp.saoEnabled[1] = bp.saoEnabled[2] = d.sao_enabled[1];
    bp.sao = (d.sao_enabled[0] || d.sao_enabled[1]) ? (const int32_t *)sl.saoCoded.p : NULL;
    bp.raw = sl.bitsRaw; bp.capPerCtu = HM_BITS_CAP_PER_CTU; bp.packed = sl.bitsPacked; bp.subSizes = sl.bitsSizes;
    bp.sync = sl.bitsSync; bp.syncFlag = sl.bitsFlag; bp.sched = L0.dSched + 8; bp.epoch = c->epoch; bp.nextInitType = d.slice_type;
    HM_CHECK(c, hipMemsetAsync(sl.bitsSizes, 0, sizeof(uint32_t) * subCap, L0.stream));     // a substream nobody coded (abandoned launch) has length 0
    if (c->sliced) {
      bp.sliceNext = (int32_t *)sl.bitsSlice.p; bp.sliceBins = sl.bitsSlice.p + numSub; bp.sliceFlag = sl.bitsSlice.p + 2 * numSub;
      HM_CHECK(c, hipMemsetAsync(sl.bitsSlice, 0, sizeof(uint32_t) * 3 * numSub, L0.stream));
    }
  }
  int rc = stage_slots(c, fbs, c->dBits, bps);
  if (rc != HM355_OK) return rc;
  // persistent grid, items handed out by ticket in dependency order (hm355_bits_kernel): any grid size drains, so the only bound is the number
  // of per-workgroup scratch areas
  unsigned int *bsched = L0.dSched + 8;
  const int total = numSub * n;
  const int grid = total < (int)L0.dWs.n ? total : (int)L0.dWs.n;
  const Params *dP = L0.dP; BitsParams *dBits = c->dBits;
  rc = timed_launches(c, 2, [&](hipStream_t s) {
    const hipError_t e = hipMemsetAsync(bsched, 0, 8, s);          // ticket = 0, abort = 0 for this launch
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hm355_bits_kernel, dim3(grid), dim3(64), 0, s, dP, dBits, n, bsched);
    hipLaunchKernelGGL(hm355_bits_pack_kernel, dim3(numSub, n), dim3(64), 0, s, dP, dBits, (const unsigned int *)bsched);
    return hipGetLastError();
  });
  if (rc != HM355_OK) return rc;
  HM_CHECK(c, hipMemcpy(bps.data(), c->dBits, sizeof(BitsParams) * n, hipMemcpyDeviceToHost));
  unsigned int bs[2] = {0, 0};
  HM_CHECK(c, hipMemcpy(bs, bsched, sizeof(bs), hipMemcpyDeviceToHost));
  if (bs[1]) return fail(c, HM355_ERR_DEVICE, "bitstream pass: a wait for the WPP hand-off or for the slice before was abandoned");
  const int numSlices = c->sliced ? numSub : 1;
  std::vector<hm355_slice_bits> sliceBits((size_t)c->slots.size() * numSlices, hm355_slice_bits());
  for (int f = 0; f < n; f++) {
    hm355_bits_desc &d = descs[f]; Slot &sl = c->slots[f];
    if (bps[f].overflow) return fail(c, HM355_ERR_DEVICE, "bitstream pass: a substream outgrew its buffer");
    HM_CHECK(c, hipMemcpy(d.sub_sizes, sl.bitsSizes, sizeof(uint32_t) * numSub, hipMemcpyDeviceToHost));
    size_t tot = 0; for (int k = 0; k < numSub; k++) tot += d.sub_sizes[k];
    if (tot > d.out_cap) return fail(c, HM355_ERR_ARG, "hm355_encode_slices_run: out_cap too small");
    if (tot) HM_CHECK(c, hipMemcpy(d.out, sl.bitsPacked, tot, hipMemcpyDeviceToHost));
    d.next_cabac_init_type = bps[f].nextInitType; d.num_bins = bps[f].bins;
    hm355_slice_bits *sb = &sliceBits[(size_t)f * numSlices];
    if (c->sliced) {
      std::vector<uint32_t> v((size_t)2 * numSub);
      HM_CHECK(c, hipMemcpy(v.data(), sl.bitsSlice, sizeof(uint32_t) * v.size(), hipMemcpyDeviceToHost));
      for (int k = 0; k < numSub; k++) { sb[k].num_substreams = 1; sb[k].next_cabac_init_type = (int32_t)v[k]; sb[k].num_bins = v[numSub + k]; }
    } else { sb[0].num_substreams = numSub; sb[0].next_cabac_init_type = bps[f].nextInitType; sb[0].num_bins = bps[f].bins; }
  }
  c->sliceBits.swap(sliceBits);
  return HM355_OK;
}

extern "C" int hm355_slice_bits_info(const hm355_ctx *c, int slot, hm355_slice_bits *out, int cap)
{
  if (!c || slot < 0 || slot >= (int)c->slots.size() || (cap > 0 && !out)) return HM355_ERR_ARG;
  const int numSlices = c->sliced ? c->slicesT.count() : 1;
  if (c->sliceBits.size() != c->slots.size() * (size_t)numSlices) return HM355_ERR_ARG;       // no bitstream pass since the partition was set
  for (int k = 0; k < numSlices && k < cap; k++) out[k] = c->sliceBits[(size_t)slot * numSlices + k];
  return numSlices;
}

// host buffers in: the CTU data of one slice goes to slot 0 first
extern "C" int hm355_encode_slice(hm355_ctx *c, hm355_bits_desc *desc, const hm355_ctu_out *ctus, const hm355_ctu_inter_out *ictus, const int32_t *sao)
{
  if (!c || !desc || !ctus) return HM355_ERR_ARG;
  if (desc->slice_type != 2 && !ictus) return fail(c, HM355_ERR_ARG, "hm355_encode_slice: inter slices need the motion data");
  if ((desc->sao_enabled[0] || desc->sao_enabled[1]) && !sao) return fail(c, HM355_ERR_ARG, "hm355_encode_slice: SAO enabled without parameters");
  Slot &sl = c->slots[0]; FrameBuf &fb = sl.fb;
  std::vector<CtuMeta> meta(c->numCtus); std::vector<TCoeff> coef((size_t)c->numCtus * HM_COEF_CTU);
  for (int a = 0; a < c->numCtus; a++) ctu_from_out(ctus[a], &meta[a], &coef[(size_t)a * HM_COEF_CTU]);
  HM_CHECK(c, hipMemcpy(fb.meta, meta.data(), sizeof(CtuMeta) * c->numCtus, hipMemcpyHostToDevice));
  HM_CHECK(c, hipMemcpy(fb.coef, coef.data(), sizeof(TCoeff) * coef.size(), hipMemcpyHostToDevice));
  if (desc->slice_type != 2) {
    HM_CHECK(c, sl.imeta.ensure(c->numCtus));
    HM_CHECK(c, hipMemcpy(sl.imeta, ictus, sizeof(InterMeta) * c->numCtus, hipMemcpyHostToDevice));
  }
  if (sao) {
    HM_CHECK(c, sl.saoCoded.ensure(c->numCtus));
    HM_CHECK(c, hipMemcpy(sl.saoCoded, sao, sizeof(SaoBlk) * c->numCtus, hipMemcpyHostToDevice));
  }
  return hm355_encode_slices_run(c, 1, desc);
}

// ------------------------------------------------------------------------------------------------
// primitive batches
// ------------------------------------------------------------------------------------------------
extern "C" int hm355_dist_batch(hm355_ctx *c, int kind, int n, int bit_depth, int count, const int16_t *org, const int16_t *cur, uint32_t *out)
{
  if (!c || !org || !cur || !out || count < 1 || kind < 0 || kind > 3 || (n != 4 && n != 8 && n != 16 && n != 32 && n != 64) || (bit_depth != 8 && bit_depth != 10)) return HM355_ERR_ARG;
  const size_t samples = (size_t)count * n * n, bytes = samples * sizeof(Pel);
  const hipStream_t s = c->lane[0].stream;
  DevBuf<Pel> dO, dC; DevBuf<uint32_t> dOut;
  if (dO.alloc(samples) != hipSuccess || dC.alloc(samples) != hipSuccess || dOut.alloc(count) != hipSuccess) return HM355_ERR_NOMEM;
  if (hipMemcpy(dO, org, bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dC, cur, bytes, hipMemcpyHostToDevice) != hipSuccess) return HM355_ERR_DEVICE;
  const int grid = count < 65536 ? count : 65536;
  hipLaunchKernelGGL(hm355_dist_kernel, dim3(grid), dim3(64), 0, s, kind, n, bit_depth, count, (const Pel *)dO.p, (const Pel *)dC.p, dOut.p);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipMemcpy(out, dOut, (size_t)count * 4, hipMemcpyDeviceToHost) != hipSuccess) { c->err = "dist kernel failed"; return HM355_ERR_DEVICE; }
  return HM355_OK;
}

extern "C" int hm355_transform_batch(hm355_ctx *c, int inverse, int n, int bit_depth, int use_dst, int count, const int32_t *in, int32_t *out)
{
  if (!c || !in || !out || count < 1 || (n != 4 && n != 8 && n != 16 && n != 32) || (bit_depth != 8 && bit_depth != 10) || (use_dst && n != 4)) return HM355_ERR_ARG;
  const size_t samples = (size_t)count * n * n, bytes = samples * 4;
  const hipStream_t s = c->lane[0].stream;
  DevBuf<int32_t> dI, dOut;
  if (dI.alloc(samples) != hipSuccess || dOut.alloc(samples) != hipSuccess) return HM355_ERR_NOMEM;
  if (hipMemcpy(dI, in, bytes, hipMemcpyHostToDevice) != hipSuccess) return HM355_ERR_DEVICE;
  const int grid = count < 65536 ? count : 65536;
  hipLaunchKernelGGL(hm355_transform_kernel, dim3(grid), dim3(64), 0, s, inverse, n, bit_depth, use_dst, count, (const int32_t *)dI.p, dOut.p);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess || hipMemcpy(out, dOut, bytes, hipMemcpyDeviceToHost) != hipSuccess) { c->err = "transform kernel failed"; return HM355_ERR_DEVICE; }
  return HM355_OK;
}
