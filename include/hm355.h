/* hm355 -- MI355X-native replacement for the CTU-level RD search of HM-16.2 (liron88/HM-16.2).
 *
 * C ABI of the drop-in boundary.  The reference has no FFI layer; the seam is the C++ member
 *     Void TEncSlice::compressSlice( TComPic* pcPic )      source/Lib/TLibEncoder/TEncSlice.h:118
 *                                                           (body TEncSlice.cpp:640-904, caller TEncGOP.cpp:1138)
 * The entry points below are what a binding of that member would call: plain pointers and sizes,
 * caller-owned buffers, blocking calls, negative return codes instead of assert/exit.
 * INTEGRATION.md shows the few lines a reference maintainer adds inside TEncSlice::compressSlice.
 *
 * All work is done by hand-written HIP kernels (hm-16.2_amd/csrc/hm355.hip + hm355_core.h).  There is NO
 * CPU fallback: without a usable gfx950 device hm355_create() fails with HM355_ERR_NO_DEVICE.
 */
#ifndef HM355_H
#define HM355_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM355_OK               0
#define HM355_ERR_ARG         -1   /* bad argument / unsupported configuration */
#define HM355_ERR_NO_DEVICE   -2   /* no HIP device or kernel image not loadable */
#define HM355_ERR_NOMEM       -3
#define HM355_ERR_DEVICE      -4   /* a HIP call or a kernel failed */

/* Sequence-level parameters: the SPS/PPS/TEncCfg getters compressSlice reads (TEncCfg.h).  The block structure is the one every cfg
 * file of the reference uses (cfg/encoder_intra_main*.cfg, encoder_lowdelay_P_main.cfg, encoder_lowdelay_main.cfg,
 * encoder_randomaccess_main*.cfg: CTU 64, depth 4, TU 4..32, RQT depth 3); other values are rejected with HM355_ERR_ARG rather than
 * silently ignored.  I, P and B slices are all accepted (the slice type is a per-call parameter). */
typedef struct {
  int32_t width, height;          /* SourceWidth/Height, multiples of 8 (min CU) */
  int32_t bit_depth;              /* InternalBitDepth 8 or 10 (luma == chroma) */
  int32_t ctu_size;               /* MaxCUWidth = 64 */
  int32_t max_cu_depth;           /* MaxPartitionDepth = 4 */
  int32_t tu_log2_max, tu_log2_min;   /* 5, 2 */
  int32_t tu_max_depth_intra;     /* QuadtreeTUMaxDepthIntra = 3 */
  int32_t wavefront_synchro;      /* WaveFrontSynchro 0/1 (TEncSlice.cpp:740-755,855-858) */
  int32_t max_batch;              /* how many independent pictures one call may carry (>=1) */
} hm355_seq_cfg;

/* Slice-level parameters: what TEncSlice::initEncSlice / setUpLambda (TEncSlice.cpp:132-159,180-481)
 * push into TComRdCost / TComTrQuant before compressSlice runs. */
typedef struct {
  int32_t slice_type;             /* 2 = I_SLICE in the I-slice entry points; the inter entry points (hm355_inter_slice_desc::base) take 1 = P_SLICE or 0 = B_SLICE */
  int32_t qp;                     /* TComSlice::getSliceQp() */
  double  lambda;                 /* TComRdCost::m_dLambda */
  double  chroma_weight;          /* TComRdCost::m_distortionWeight[Cb]==[Cr] */
} hm355_slice_desc;

/* planar 4:2:0 picture, 16-bit samples, tightly packed rows (stride == width of the plane) */
typedef struct {
  uint16_t *plane[3];
} hm355_planes;

/* Per-CTU result: the TComDataCU arrays compressSlice leaves in pcPic->getCtu(rs)
 * (TComDataCU.h:86-157), 256 4x4 partitions in z-scan order, and m_pcTrCoeff in HM's TU packing
 * (TU with z-order index z starts at z*16 for luma, z*4 for chroma; row-major inside the TU). */
typedef struct {
  double   total_cost;            /* m_dTotalCost */
  uint32_t total_bits;            /* m_uiTotalBits */
  uint32_t total_dist;            /* m_uiTotalDistortion */
  uint8_t  depth[256], part_size[256], pred_mode[256], intra_dir_luma[256], intra_dir_chroma[256],
           tr_idx[256], cbf[3][256], tskip[3][256];
  int32_t  coeff_y[4096], coeff_cb[1024], coeff_cr[1024];
} hm355_ctu_out;

/* m_uiPicTotalBits / m_dPicRdCost / m_uiPicDist (TEncSlice.cpp:889-891) */
typedef struct {
  uint64_t pic_total_bits;
  double   pic_rd_cost;
  uint64_t pic_dist;
} hm355_slice_stats;

typedef struct hm355_ctx hm355_ctx;

/* TEncTop::create/init equivalent for the hot path: allocates every device buffer once. */
int  hm355_create(const hm355_seq_cfg *cfg, hm355_ctx **out);
void hm355_destroy(hm355_ctx *ctx);
const char *hm355_last_error(const hm355_ctx *ctx);
/* identifies the kernel source this library was built from (hash of hm-16.2_amd/csrc + this header): measurement records carry it */
const char *hm355_build_id(void);

/* Replacement of TEncSlice::compressSlice for one picture (host buffers in, host buffers out).
 *   org  : TComPic::getPicYuvOrg()          rec : TComPic::getPicYuvRec() (pre-deblocking)
 *   ctus : one record per CTU, raster order  stats : may be NULL */
int hm355_compress_slice(hm355_ctx *ctx, const hm355_slice_desc *slice, const hm355_planes *org,
                         hm355_planes *rec, hm355_ctu_out *ctus, hm355_slice_stats *stats);

/* The same for n independent pictures (all-intra: every picture is an IDR-like I slice with its own
 * CABAC reset, TEncSlice.cpp:653-654), evaluated concurrently.  n <= max_batch. */
int hm355_compress_slices(hm355_ctx *ctx, int n, const hm355_slice_desc *slices, const hm355_planes *org,
                          hm355_planes *rec, hm355_ctu_out *const *ctus, hm355_slice_stats *stats);

/* ---- P and B slices (encoder_lowdelay_P_main.cfg, encoder_lowdelay_main.cfg, encoder_randomaccess_main*.cfg): the reference
 * pictures and slice-header values that TEncSlice::compressSlice finds through pcSlice->getRefPic(list, idx) / TComSlice
 * getters are inputs.  Replaces the same member for inter slices: merge / skip, AMVP, TZ integer search + fractional
 * refinement (TEncSearch::predInterSearch / xMotionEstimation, TEncSearch.cpp:3075-3906), bi-prediction search
 * (xPatternSearch :3932, GPB shortcut, mvd_l1_zero), AMP, inter RQT (xEstimateResidualQT :4680) and the intra candidates of
 * inter slices.  Weighted prediction off, FEN on (one bi-prediction iteration), as in the reference's cfg files. ---- */
typedef struct {
  int32_t poc, slice_type, long_term;
  const uint16_t *plane[3];           /* TComPic::getPicYuvRec() after the loop filters, tightly packed */
  const uint8_t *pred_mode;           /* motion field after TComPic::compressMotion: [numCtus*256] */
  const int16_t *mv[2];               /* [numCtus*256*2] (x, y), quarter samples */
  const int8_t *ref_idx[2];           /* [numCtus*256] */
  int32_t num_ref[2], ref_poc[2][16], ref_lt[2][16];   /* reference lists that picture was coded with (TMVP scaling) */
} hm355_ref_pic;
struct hm355_ref;
typedef struct {
  hm355_slice_desc base;              /* slice_type 1 (P) or 0 (B), qp, lambda, chroma weight */
  int32_t poc;
  int32_t cabac_init_type;            /* context table in use (TEncSbac::resetEntropy, TEncSbac.cpp:106-115): 0 = B, 1 = P */
  int32_t num_ref_idx[2];
  const hm355_ref_pic *ref[2][16];
  int32_t col_from_l0, col_ref_idx, tmvp, mvd_l1_zero, max_merge_cand, check_ldc;
  uint32_t lambda_motion_sad, lambda_motion_sse;       /* TComRdCost::m_uiLambdaMotionSAD / SSE[0] */
  const struct hm355_ref *dev_ref[2][16];              /* device-resident alternative to ref[l][i] (hm355_ref_from_slot); used when non-NULL */
} hm355_inter_slice_desc;
/* per-CTU motion data: m_skipFlag, m_pbMergeFlag, m_puhMergeIndex, m_puhInterDir, m_acCUMvField[2] (mv, mvd, refIdx),
 * m_apiMVPIdx / m_apiMVPNum (TComDataCU.h:86-157) */
typedef struct {
  uint8_t skip[256], merge_flag[256], merge_idx[256], inter_dir[256];
  int16_t mv[2][256][2], mvd[2][256][2];
  int8_t  ref_idx[2][256], mvp_idx[2][256], mvp_num[2][256];
} hm355_ctu_inter_out;
int hm355_compress_slice_inter(hm355_ctx *ctx, const hm355_inter_slice_desc *slice, const hm355_planes *org,
                               hm355_planes *rec, hm355_ctu_out *ctus, hm355_ctu_inter_out *ictus, hm355_slice_stats *stats);
/* n P pictures that do not reference each other (the current pictures of n streams, or of n independent GOP chains),
 * evaluated concurrently; a hm355_ref_pic named by several slices is uploaded once.  n <= max_batch. */
int hm355_compress_slices_inter(hm355_ctx *ctx, int n, const hm355_inter_slice_desc *slices, const hm355_planes *org,
                                hm355_planes *rec, hm355_ctu_out *const *ctus, hm355_ctu_inter_out *const *ictus, hm355_slice_stats *stats);

/* ---- device-resident reference pictures: the finished picture of a slot (after hm355_deblock_run) becomes a reference without a
 * host round trip: border extension (TComPicYuv::extendPicBorder, TComPicYuv.cpp:171) and TComPic::compressMotion (TEncGOP.cpp:1660)
 * run on the device.  is_inter = 0 for an I picture (no motion), else the slot's motion data of its last hm355_compress_slices_inter;
 * num_ref / ref_poc / ref_lt = the reference lists that picture was coded with (TMVP scaling).  The slot can be reused afterwards. ---- */
typedef struct hm355_ref hm355_ref;
int hm355_ref_from_slot(hm355_ctx *ctx, int slot, int32_t poc, int32_t is_inter, const int32_t num_ref[2], const int32_t ref_poc[2][16],
                        const int32_t ref_lt[2][16], hm355_ref **out);
void hm355_ref_release(hm355_ctx *ctx, hm355_ref *ref);
/* The same reference picture as ONE blob of hm355_ref_bytes() bytes (header, border-extended planes, compressed motion field), in host or
 * device memory: what crosses devices when pictures of one temporal layer are searched on different GPUs and the finished pictures are
 * all-gathered (SURVEY.md 8e "Inter"; TEncGOP.cpp:1184,1483,1660 make a picture a reference only after deblocking, SAO and
 * compressMotion, which is the state hm355_ref_from_slot captures).  A device buffer goes to RCCL as it is (hm-16.2_amd/gop_shard.py).
 * user[4]: four doubles that travel with the picture (the scheduler's per-picture state, e.g. the SAO disabled rates); may be NULL. */
size_t hm355_ref_bytes(const hm355_ctx *ctx);
int hm355_ref_export(hm355_ctx *ctx, const hm355_ref *ref, void *buf, const double user[4]);
int hm355_ref_import(hm355_ctx *ctx, const void *buf, hm355_ref **out, double user[4]);

/* ---- deblocking filter: TComLoopFilter::loopFilterPic (TLibCommon/TComLoopFilter.cpp:130-158), the step TEncGOP runs after
 * compressSlice (TEncGOP.cpp:1184) to turn the reconstruction into a reference picture.  Deblocking offsets 0, one slice,
 * no PCM / lossless (every cfg of the reference); SAO is a separate, later stage. ---- */
typedef struct {
  int32_t slice_type, qp;             /* slice QP (no delta QP: every CU carries it) */
  int32_t ref_poc[2][16];             /* POC of the slice's reference pictures [list][idx]: boundary strength compares pictures */
} hm355_dbk_desc;
/* host buffers: rec (the pre-deblocking reconstruction compressSlice left) is filtered in place, using ctus / ictus of the same slice
 * (ictus may be NULL for an I slice) */
int hm355_deblock(hm355_ctx *ctx, const hm355_dbk_desc *desc, const hm355_ctu_out *ctus, const hm355_ctu_inter_out *ictus, hm355_planes *rec);
/* device-resident: filters the reconstruction of slots 0..n-1 in place, right after hm355_run / hm355_compress_slices(_inter) left
 * their per-CTU data there; hm355_download then returns the deblocked picture */
int hm355_deblock_run(hm355_ctx *ctx, int n, const hm355_dbk_desc *descs);

/* ---- sample adaptive offset, encoder side: TEncSampleAdaptiveOffset::SAOProcess (TEncGOP.cpp:1483) on the deblocked pictures of slots
 * 0..n-1 (after hm355_deblock_run), against the originals uploaded to the same slots: statistics, picture-level on/off, per-CTU
 * off / new / merge decision with the SAO syntax on the CABAC estimator, offsets applied in place.  One slice, no tiles,
 * SAOLcuBoundary 0, offset bit shifts 0 (every cfg of the reference). ---- */
typedef struct {
  int32_t qp, cabac_init_type, depth;  /* slice QP; context table of the slice (0 B, 1 P, 2 I); temporal depth (TComSlice::getDepth) */
  double lambda, chroma_weight;        /* TComSlice::getLambdas(): luma lambda, chroma lambda = lambda / chroma_weight */
  double disabled_rate[3][8];          /* in/out: TEncSampleAdaptiveOffset::m_saoDisabledRate[component][depth], carried from picture to picture */
  int32_t enabled[3];                  /* out: slice-level SAO flags (luma, Cb, Cr) */
  int32_t *params;                     /* out, may be NULL: numCtus x 3 x 35 int32 (modeIdc, typeIdc, typeAuxInfo, offset[32]) as coded */
} hm355_sao_desc;
int hm355_sao_run(hm355_ctx *ctx, int n, hm355_sao_desc *descs);

/* ---- bitstream pass: TEncSlice::encodeSlice (TEncSlice.cpp:910-1095, called from TEncGOP.cpp:1559) on the pictures of slots 0..n-1 as
 * the search (hm355_run / hm355_compress_slices_inter) and, when sao_enabled is set, hm355_sao_run left them: the CABAC-coded slice data,
 * one substream per CTU row with WPP, else one.  Each substream ends with the terminating bin, the CABAC flush (TEncBinCABAC::finish)
 * and the byte alignment -- exactly the bytes TEncGOP.cpp:1572-1583 concatenates behind the slice header, before emulation prevention;
 * sub_sizes are the entry point sizes of the slice header (TEncSlice.cpp:1067-1071 adds the emulation count).  Slice header, parameter
 * sets and NAL packing stay with the caller. ---- */
typedef struct {
  int32_t slice_type, qp;              /* 2 = I, 1 = P, 0 = B; slice QP */
  int32_t cabac_init_type;             /* context table of a P / B slice (TEncSbac::resetEntropy :106-115); ignored for I */
  int32_t num_ref_idx[2], mvd_l1_zero, max_merge_cand;   /* slice header values the PU syntax depends on (P / B) */
  int32_t sao_enabled[2];              /* slice_sao_luma_flag, slice_sao_chroma_flag: both 0 = no SAO syntax (SPS SAO off, or switched off for the slice) */
  uint8_t *out; size_t out_cap;        /* out: the substreams back to back */
  uint32_t *sub_sizes;                 /* out: [hm355_num_substreams()] bytes of each substream */
  int32_t next_cabac_init_type;        /* out: TEncSbac::determineCabacInitIdx (:163-222): the table the PPS carries for the following pictures */
  uint32_t num_bins;                   /* out: bins coded (TEncBinCABAC::getBinsCoded) */
} hm355_bits_desc;
int hm355_num_substreams(const hm355_ctx *ctx);
int hm355_encode_slices_run(hm355_ctx *ctx, int n, hm355_bits_desc *descs);
/* host buffers in: the CTU data of one slice in the layout the search returns it (ictus NULL for an I slice), sao = numCtus x 3 x 35 int32 as
 * hm355_sao_run returns them (NULL with sao_enabled 0).  Uses slot 0. */
int hm355_encode_slice(hm355_ctx *ctx, hm355_bits_desc *desc, const hm355_ctu_out *ctus, const hm355_ctu_inter_out *ictus, const int32_t *sao);

/* ---- picture statistics: what TEncGOP::compressGOP does with the finished picture -- TEncGOP::xCalculateAddPSNR (TEncGOP.cpp:2244-2368, called
 * at :1725 for every picture) and the decoded picture hash of --SEIDecodedPictureHash (TEncGOP.cpp:1665-1696; TComPicYuvMD5.cpp calcMD5 / calcCRC /
 * calcChecksum) -- on the device, so that only a few bytes per picture cross PCIe.  The SSD original - reconstruction runs per component over the
 * picture without its right / bottom padding (TEncCfg::m_aiPad); the hash runs over the whole coded plane.  PSNR and MSE are the reference's double
 * expressions (:2287-2290), evaluated on the host from the 64-bit SSD.  digest holds digest_len bytes per component in the order
 * TComDigest::hash holds them (MD5: the 16 digest bytes; CRC: 2 bytes, high first; checksum: 4 bytes, high first); the SEI writer stays with
 * the caller.  4:2:0; no colour-space-converted PSNR, no field PSNR. ---- */
typedef struct {
  int32_t hash_method;                 /* 0 none, 1 MD5, 2 CRC, 3 checksum (--SEIDecodedPictureHash) */
  int32_t pad_right, pad_bottom;       /* luma samples of TEncCfg::m_aiPad[0] / [1] (even, smaller than the picture): excluded from SSD / PSNR, included in the hash */
  uint64_t ssd[3];                     /* out */
  double   psnr[3], mse[3];            /* out */
  uint8_t  digest[3][16];              /* out: digest_len bytes per component */
  int32_t  digest_len;                 /* out: 16 / 2 / 4, 0 with hash_method 0 */
} hm355_picstat_desc;
/* device-resident: slots 0..n-1, the reconstruction as it stands (after hm355_sao_run: the finished picture) against the slots' originals.
 * Reads the slots only: nothing a later call sees is changed. */
int hm355_picture_stats_run(hm355_ctx *ctx, int n, hm355_picstat_desc *descs);
/* host buffers in (uses slot 0: its original and reconstruction planes are overwritten), the drop-in form next to hm355_deblock */
int hm355_picture_stats(hm355_ctx *ctx, hm355_picstat_desc *desc, const hm355_planes *org, const hm355_planes *rec);
/* host -> the reconstruction planes of a slot: a picture that was reconstructed elsewhere, next to hm355_upload for its original, so that
 * hm355_picture_stats_run can take a batch of them */
int hm355_upload_rec(hm355_ctx *ctx, int slot, const hm355_planes *rec);

/* ---- picture ingest and output: TVideoIOYuv::read / ::write (TVideoIOYuv.cpp:633-792) for planar 4:2:0 files, as TAppEncTop::encode drives them
 * (:431 read into the padded source picture, :603 write of the reconstruction with the conformance window).  The frames travel as they are on
 * disk (8-bit samples, or 16-bit little endian when file_bit_depth > 8); bit-depth scaling, padding by repetition up to the configured
 * (padded) width x height, cropping, rounding and clipping happen on the device.
 * hm355_upload_file_frames: frames[i] -> original planes of slot i.  hm355_download_file_frames: the reconstruction (source 0) or the original
 * planes (source 1) of slot i -> frames[i] of (width - conf_right) x (height - conf_bottom) samples at file_bit_depth.
 * hm355_download_org: the original planes of a slot as the encoder sees them (the TComPicYuv view of the padded source picture). ---- */
int hm355_upload_file_frames(hm355_ctx *ctx, int n, const void *const *frames, int file_width, int file_height, int file_bit_depth);
int hm355_download_file_frames(hm355_ctx *ctx, int n, void *const *frames, int file_bit_depth, int conf_right, int conf_bottom, int source);
int hm355_download_org(hm355_ctx *ctx, int slot, hm355_planes *org);

/* ---- cu_qp_delta: the hooks adaptive QP and rate control have inside compressSlice (TEncSlice.cpp:767-808 hands the CTU its QP through
 * TEncRateCtrl::setRCQP, TEncCu::xComputeQP :1154 derives it from the TEncPreanalyzer activities; TEncCu::xCheckDQP :1742, the split candidate
 * :1052-1085 and TEncEntropy.cpp:343-351 price / code the delta QP; TComDataCU::m_phQP feeds the deblocking filter).  MaxCuDQPDepth 0 (the CTU
 * is the quantisation group), MaxDeltaQP 0.  hm355_set_dqp arms a slot: its following searches (hm355_run*, hm355_compress_slice(s)(_inter)),
 * hm355_deblock_run and hm355_encode_slices_run run with cu_qp_delta enabled until it is called again with NULL / use_dqp 0.
 * hm355_get_dqp returns what the search left: m_phQP of every CTU ([numCtus*256]) and TEncCu::m_bEncodeDQP (input of the next picture).
 * hm355_preanalyze: TEncPreanalyzer::xPreanalyze (TEncPreanalyzer.cpp:64) for layer 0 on the slot's original picture -- the integer part on
 * the device: sums[a*8 + 0..3] = sum, [4..7] = sum of squares of the luma samples of CTU a's four quadrants; the caller derives the activities
 * and the QP offsets in double precision as the reference does (hm-16.2_amd/host/TEncTop.cpp, hm-16.2_amd/hm355.py aq_ctu_qp). ---- */
typedef struct {
  int32_t use_dqp;                     /* PPS cu_qp_delta_enabled_flag */
  int32_t dqp_flag_in;                 /* TEncCu::m_bEncodeDQP on entry (what the previous picture's encodeSlice left) */
  const int8_t *ctu_qp;                /* [numCtus] QP of every CTU; NULL: the slice QP (picture-level rate control) */
} hm355_dqp_desc;
int hm355_set_dqp(hm355_ctx *ctx, int slot, const hm355_dqp_desc *desc);
int hm355_get_dqp(hm355_ctx *ctx, int slot, int8_t *qp_out, int32_t *dqp_flag_out);
int hm355_preanalyze(hm355_ctx *ctx, int slot, uint64_t *sums);

/* ---- LCU-level rate control (--RateControl=1, LCULevelRateControl on: TEncSlice.cpp:766-887).  Before each CTU the caller's rate model
 * (TEncRateCtrl, which stays with the caller) gives it a lambda and a QP; after it, updateAfterCTU takes the CTU's bits and QP -- so the QP of
 * CTU n depends on the bits of CTUs 0..n-1, and the slice is searched CTU range by CTU range with the model in between.
 * hm355_set_ctu_rc: QP and lambda of CTUs [first_ctu, first_ctu + n) of a slot armed with hm355_set_dqp (use_dqp 1); QPs in [-QpBDOffset, 51],
 * lambdas in [1e-4, 65535] (what the motion lambda's 32 bits hold; TEncRateCtrl clips to [0.1, 10000]); lambda NULL: the slice lambda.  What TComRdCost::setLambda / TComTrQuant::setLambdas derive from a lambda (its
 * square root, the chroma lambda = lambda / the slice's chroma weight, the motion lambdas, the sign-hiding factor of the CTU's QP) is computed on
 * the host in double precision.  Honoured by every search entry on that slot (hm355_run, hm355_compress_slice(s)(_inter), hm355_run_ctus) until
 * hm355_set_dqp is called again.
 * Slice-resident search: hm355_slice_begin (I) / hm355_slice_begin_inter (P / B; device-resident references dev_ref only) opens a slice on an
 * armed slot (hm355_set_dqp first; it is refused while the slice is open) whose original is already in HBM (hm355_upload, hm355_upload_file_frames);
 * hm355_run_ctus searches CTUs [first_ctu, first_ctu + num_ctus) in coding order in slots [first_slot, first_slot + n), one launch: first_ctu must
 * equal the number of CTUs already searched in the slice (hm355_slice_begin* sets it to 0).  Under WaveFrontSynchro the first CTU of a row takes the real
 * m_bEncodeDQP of the CTU an earlier call finished.  hm355_ctu_rc_feedback reads back 8 bytes per CTU: getTotalBits() and getQP(0), or -999
 * (g_RCInvalidQPValue) when no partition inside the picture is coded other than skip -- for CTUs the last search of the slot's picture (any search
 * entry; an upload starts a new picture) reached with the slot armed.
 * hm355_download / hm355_download_inter return the CTU data; after hm355_slice_end the slot allows what a slot searched by
 * hm355_compress_slices_inter allows (hm355_deblock_run, hm355_sao_run, hm355_encode_slices_run, hm355_ref_from_slot).  Lane 0.
 * hm355_intra_cost: TEncSlice::calCostSliceI (TEncSlice.cpp:606-632) on the slot's original luma: cost[a] = m_costIntra of CTU a (the sum of
 * the 8x8 Hadamard costs of the whole 8x8 blocks inside the picture, rounded to 8 bits), what TEncRCPic::setTotalIntraCost adds up before an
 * I picture. ---- */
typedef struct { int32_t bits; int32_t qp; } hm355_ctu_rc;     /* pCtu->getTotalBits(); pCtu->getQP(0) or -999 */
int hm355_set_ctu_rc(hm355_ctx *ctx, int slot, int first_ctu, int n, const int8_t *qp, const double *lambda);
int hm355_slice_begin(hm355_ctx *ctx, int slot, const hm355_slice_desc *sd);
int hm355_slice_begin_inter(hm355_ctx *ctx, int slot, const hm355_inter_slice_desc *sd);
int hm355_run_ctus(hm355_ctx *ctx, int first_slot, int n, int first_ctu, int num_ctus);
int hm355_ctu_rc_feedback(hm355_ctx *ctx, int slot, int first_ctu, int n, hm355_ctu_rc *out);
int hm355_download_inter(hm355_ctx *ctx, int slot, hm355_ctu_inter_out *ictus);
int hm355_slice_end(hm355_ctx *ctx, int slot);
int hm355_intra_cost(hm355_ctx *ctx, int slot, int32_t *cost);

/* ---- device-resident variant (what bench.py times: inputs already in HBM) ----
 * Upload / run / download are separate so that a caller can keep pictures resident. */
int hm355_upload(hm355_ctx *ctx, int slot, const hm355_planes *org);          /* host -> HBM picture slot */
int hm355_run(hm355_ctx *ctx, int n, const hm355_slice_desc *slices);         /* slots [0,n) -> results in HBM; blocking */
int hm355_download(hm355_ctx *ctx, int slot, hm355_planes *rec, hm355_ctu_out *ctus, hm355_slice_stats *stats);
/* Pipelined steps (the calling pattern of TEncGOP::compressGOP -> compressSlice, TEncGOP.cpp:1138, for a caller that keeps several groups
 * of independent pictures in flight): hm355_run_begin enqueues the search over slots [first_slot, first_slot + n) on pipeline lane
 * `lane` (0..3) and returns; hm355_run_wait blocks until that lane's launch has finished and reports its kernel time (HIP events on the
 * lane's stream) and errors.  Launches of different lanes run concurrently, each with its own stream and scratch areas, so the
 * wavefront drain of one group overlaps the fill of the next; slot ranges of launches in flight must not overlap.  I slices. */
int hm355_run_begin(hm355_ctx *ctx, int lane, int first_slot, int n, const hm355_slice_desc *slices);
/* how many launches the caller keeps in flight (1..4, default 1): each then takes that share of the device's resident searches, so that they
 * run side by side instead of one after the other (a waiting persistent workgroup keeps its place on the CU) */
int hm355_set_lane_share(hm355_ctx *ctx, int launches_in_flight);
int hm355_run_wait(hm355_ctx *ctx, int lane, double *kernel_ms);
/* The reference's fast encoder decisions for P / B slices, each 0 or 1 (default 0 / 0 / 0): --ESD early skip detection (TEncCu.cpp:630-643, :657,
 * :1497-1525: the 2Nx2N search runs before the merge check; a best mode without residual that is a merge or has a zero MVD ends the CU's candidates),
 * --CFM CBF fast mode (:644-647 .. :798: no further inter shape once the running best has no residual) and --ECU early CU (:867-874, :980: a CU
 * whose best mode is a skip is not split).  The state is sticky and belongs to the context: it applies to every later search of a P / B slice
 * (hm355_compress_slice(s)_inter, hm355_slice_begin_inter + hm355_run_ctus); I slices ignore it, whichever entry point searches them.  With any switch on, a P / B launch is searched by one wavefront per CTU (no wavefront teams, whatever HM355_TEAM says).
 * HM355_ERR_ARG: a value other than 0 or 1; a slice open on any slot; a hm355_run_begin launch outstanding. */
int hm355_set_fast_decisions(hm355_ctx *ctx, int esd, int cfm, int ecu);
/* The reference's integer motion search of P / B slices (TEncSearch.cpp:215-217, :3829-3831, :3872): --FastSearch (1: TZ, 0: the exhaustive
 * xPatternSearch for uni-prediction too), --SearchRange 1..256 and --BipredSearchRange 1..16; defaults 1 / 64 / 4.  Sticky, per context, and
 * followed by every later search of a P / B slice like hm355_set_fast_decisions; I slices ignore it.  With fast_search 0 a P / B launch is
 * searched by one wavefront per CTU (no wavefront teams, whatever HM355_TEAM says).  Not built and rejected: FastSearch=2 (the selective TZ
 * search, :4016); ASR, the adaptive search range, has no parameter here -- a caller whose configuration turns it on must not bind.
 * HM355_ERR_ARG with a message in hm355_last_error: any other value; a slice open on any slot; a hm355_run_begin launch outstanding.  A
 * rejected call leaves the previous setting in force. */
int hm355_set_motion_search(hm355_ctx *ctx, int fast_search, int search_range, int bipred_search_range);
/* Tiles (PPS tiles_enabled_flag; TComPicSym::initTiles, TComPicSym.cpp:198-300): num_cols x num_rows tiles, col_width_ctus[num_cols] and
 * row_height_ctus[num_rows] in CTUs (all entries, the last ones included).  Sticky and per context like hm355_set_motion_search; 1 x 1 turns
 * tiles off, which is the state after hm355_create.  The CTUs of a tiled picture are coded tile after tile (tile scan), every tile starts
 * with fresh CABAC contexts, and a neighbour in another tile is unavailable to the intra reference samples, the most probable modes, the split
 * and skip flag contexts, the spatial merge / AMVP candidates and the SAO merge candidates; the temporal candidate, the motion search window and
 * -- lf_cross_tile 1, LFCrossTileBoundaryFlag -- deblocking and the SAO sample classification cross tile edges.  The results stay in raster order;
 * hm355_num_substreams() becomes num_cols * num_rows and the bitstream pass returns one substream per tile, in tile order.  Every tile is a
 * chain of CTU searches of its own, so one picture offers num_cols * num_rows CTUs at a time.
 * HM355_ERR_ARG with a message in hm355_last_error, the previous layout staying in force: widths / heights that do not sum to the picture's size
 * in CTUs; a column narrower than 4 CTUs or a row lower than 1 (Main / Main10: a tile is at least 256 x 64 luma samples); more than 20 columns
 * or 22 rows; lf_cross_tile other than 1 (not built); a context with WaveFrontSynchro (Main / Main10 refuse tiles with it); cu_qp_delta armed on
 * a slot; a slice open on any slot; a hm355_run_begin launch outstanding.  While tiles are on, hm355_set_dqp (arming), hm355_run_rows,
 * hm355_export_boundary / hm355_import_boundary, hm355_slice_begin(_inter) and hm355_run_ctus are refused: their CTU ranges are raster
 * addresses and their predictors follow the untiled coding order. */
int hm355_set_tiles(hm355_ctx *ctx, int num_cols, const int *col_width_ctus, int num_rows, const int *row_height_ctus, int lf_cross_tile);
/* uniform tile spacing (uniform_spacing_flag): column c of num_cols is (c + 1) * w_ctu / num_cols - c * w_ctu / num_cols CTUs wide, rows alike */
void hm355_uniform_tiles(int w_ctu, int h_ctu, int num_cols, int num_rows, int *col_width_ctus, int *row_height_ctus);
/* Slices (TEncSlice::compressSlice / encodeSlice once per slice, TEncGOP.cpp:1135-1166, :1559): num_slices slices, first_ctu[num_slices] the raster
 * address of the first CTU of each, ascending from first_ctu[0] == 0.  Sticky and per context like hm355_set_tiles; one slice turns slices off,
 * which is the state after hm355_create.  Every slice starts with fresh CABAC contexts, and a neighbouring CTU that belongs to another slice is
 * unavailable to the intra reference samples, the most probable modes, the split and skip flag contexts, the spatial merge / AMVP candidates and
 * the SAO merge candidates (TComDataCU::CUIsFromSameSliceAndTile); the temporal candidate, the motion search window and -- lf_cross_slice 1,
 * LFCrossSliceBoundaryFlag -- deblocking and the SAO sample classification cross slice edges.  The results stay in raster order and
 * hm355_slice_stats stays per picture.  hm355_num_substreams() becomes num_slices and the bitstream pass returns one substream per slice, in coding
 * order; slice k > 0 of a P / B picture is coded from the context table slice k - 1 chose, only slice 0 from the desc's cabac_init_type; in
 * hm355_bits_desc next_cabac_init_type is the last slice's and num_bins the sum, hm355_slice_bits_info has the values of every slice.  Every slice
 * is a chain of CTU searches of its own, so one picture offers num_slices CTUs at a time.
 * HM355_ERR_ARG with a message in hm355_last_error, the previous partition staying in force: a list that is not ascending from 0 or reaches past
 * the picture; lf_cross_slice other than 1 (not built); a context with WaveFrontSynchro (not built yet; the reference then ends a slice that
 * starts inside a CTU row with that row, and a list that breaks this rule is refused for that reason first); tiles in force (and hm355_set_tiles
 * while slices are in force); cu_qp_delta armed on a slot; a slice open on any slot; a hm355_run_begin launch outstanding.  While slices are on,
 * hm355_set_dqp (arming), hm355_run_rows, hm355_export_boundary / hm355_import_boundary, hm355_slice_begin(_inter) and hm355_run_ctus are refused
 * as with tiles.
 * Out of scope: SliceMode=2 (a byte budget per slice needs the bits of every CTU fed back before the next one starts), SliceMode=3 (whole tiles
 * per slice), dependent slice segments (SliceSegmentMode), and the level limits on the number of slices, which are the caller's business. */
int hm355_set_slices(hm355_ctx *ctx, int num_slices, const int *first_ctu, int lf_cross_slice);
/* SliceMode=1 (--SliceMode=1 --SliceArgument=ctus_per_slice; TEncSlice::calculateBoundingCtuTsAddrForSlice): a new slice every ctus_per_slice
 * CTUs; with wpp (WaveFrontSynchro) a slice that starts inside a CTU row ends with that row at the latest.  Returns the number of slices (0: bad
 * arguments) and writes the first CTU of the first `cap` of them. */
int hm355_fixed_ctu_slices(int w_ctu, int h_ctu, int wpp, int ctus_per_slice, int *first_ctu_out, int cap);
int hm355_num_slices(const hm355_ctx *ctx);
/* what the last hm355_encode_slices_run / hm355_encode_slice left for every slice of the picture in `slot`: returns the number of slices and
 * writes the first `cap` entries (one entry, the picture's, without slices) */
typedef struct { int32_t num_substreams; int32_t next_cabac_init_type; uint32_t num_bins; } hm355_slice_bits;
int hm355_slice_bits_info(const hm355_ctx *ctx, int slot, hm355_slice_bits *out, int cap);

/* CTU-row bands (TEncSlice.cpp:740-755,855-858 are the WPP hand-off points a band boundary cuts through): a picture is
 * searched by several devices, each owning a band of whole CTU rows [first_row, last_row] of the pictures in slots
 * [first_slot, first_slot + n) (WaveFrontSynchro=1, I slices).  The rows above first_row must be complete in the slot: searched by an
 * earlier hm355_run_rows on this context, or -- the row right above -- brought in with hm355_import_boundary from the device that owns it.
 * hm355_export_boundary copies out what the band below reads from CTU row `row`: the bottom sample line of the three planes (intra
 * reference samples, TComPattern.cpp:107-165), the CTUs' decision arrays (split-flag contexts, TComDataCU.cpp:1587) and the CABAC
 * state after each CTU (the WPP synchronisation source, TEncSlice.cpp:855-858); hm355_boundary_bytes() bytes per picture.  The buffers
 * may be host or device memory (the copies are address-space agnostic): a device buffer is handed to RCCL send / recv as it is, so a
 * boundary row never touches the host (bench.py --shard rows, hm-16.2_amd/bands.py).  The transport between devices is the caller's. */
int hm355_run_rows(hm355_ctx *ctx, int first_slot, int n, const hm355_slice_desc *slices, int first_row, int last_row);
size_t hm355_boundary_bytes(const hm355_ctx *ctx);
int hm355_export_boundary(hm355_ctx *ctx, int slot, int row, void *buf);
int hm355_import_boundary(hm355_ctx *ctx, int slot, int row, const void *buf);
/* kernel time of the last hm355_run in milliseconds, measured with HIP events on the launch stream,
 * and the number of kernel launches it took */
int hm355_last_run_info(const hm355_ctx *ctx, double *kernel_ms, int *launches);
/* The shape of the last search launch on lane 0 (hm355_run, hm355_run_rows, hm355_run_ctus, hm355_compress_slice(s)(_inter), hm355_run_begin with
 * lane 0), for tests and tuning runs that must know which code path they measured.  It is the FIRST launch of the call: the one-slot launches
 * with which a cu_qp_delta search under WaveFrontSynchro repeats rows afterwards do not replace it.  All zero before the first search. */
typedef struct hm355_launch_shape {
  int32_t kernel;      /* 0: one wavefront per CTU search, 12 searches per workgroup; 1: a team of wavefronts per CTU search */
  int32_t waves;       /* wavefronts per workgroup: 12, or the wavefronts of a team (5: I slices, 9: P / B slices) */
  int32_t few_waves;   /* 1: the launch cannot fill the device and runs the code path with the shortest dependency chain; 0: the one with the fewest instructions */
  int32_t workgroups;  /* workgroups launched */
  int32_t tickets;     /* CTU searches of the launch */
} hm355_launch_shape;
int hm355_last_launch_shape(const hm355_ctx *ctx, hm355_launch_shape *out);

/* ---- distortion / transform primitives as batched kernels (TComRdCost.cpp:465-1606,
 *      TComTrQuant.cpp:836-935); used by the known-answer parity tests and micro-benchmarks ----
 * blocks are n x n, tightly packed, `count` of them back to back. kind: 0 SAD, 1 SSE, 2 SATD */
int hm355_dist_batch(hm355_ctx *ctx, int kind, int n, int bit_depth, int count,
                     const int16_t *org, const int16_t *cur, uint32_t *out);
int hm355_transform_batch(hm355_ctx *ctx, int inverse, int n, int bit_depth, int use_dst, int count,
                          const int32_t *in, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
