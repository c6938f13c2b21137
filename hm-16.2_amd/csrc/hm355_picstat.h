// hm355 picture statistics: what TEncGOP::compressGOP does with the finished picture (TEncGOP.cpp:1665-1696, :1725) -- the 64-bit sum of squared
// differences original - reconstruction per component behind the log's PSNR (xCalculateAddPSNR, TEncGOP.cpp:2244-2368) and the decoded picture
// hash of --SEIDecodedPictureHash (TComPicYuvMD5.cpp: calcMD5, calcCRC, calcChecksum) -- on the pictures resident in the slots.  Integer
// arithmetic only; workgroups combine by integer add / xor atomics, so no result depends on the order of arrival.
//   hm355_picstat_kernel  SSD over the unpadded area and, with hash method 3, the checksum over the whole coded plane: one streaming pass
//   hm355_crc_kernel      hash method 2.  A launch of its own: it reads the reconstruction only and covers the whole coded plane, while the
//                         SSD covers the unpadded area of both pictures; apart, methods 0 / 1 / 3 do not pay the CRC's ALU work
//   hm355_md5_kernel      hash method 1: one lane per (picture, component) chain
// The arithmetic (everything above the kernels) is plain C++ that also compiles without HIP under HM355_HOSTSIM: tests/hostsim/hostsim_picstat.cpp
// walks the same partition of the planes in plain loops.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(HM355_HOSTSIM)
#define HM_PS_FN static inline
#else
#define HM_PS_FN __host__ __device__ __forceinline__
#endif

struct PicStatParams { int32_t hashMethod, padRight, padBottom, pad; };   // one picture of the batch (hm355_picstat_desc)
struct PicStatAcc {                   // what the kernels leave for one picture; zero before the launches
  unsigned long long ssd[3];
  uint32_t cksum[3], crc[3];          // crc: the XOR of the chunks' terms (the host adds the term of the initial value)
  uint32_t md5[3][4];                 // the chains' final states A, B, C, D
};

// ---- SSD and checksum: the terms of one sample ----
HM_PS_FN uint32_t ps_ssd_term(int org, int rec) { const int d = org - rec; const uint32_t a = (uint32_t)(d < 0 ? -d : d); return a * a; }
// compChecksum: every byte of the sample XORed with an 8-bit mask of its position, summed mod 2^32
HM_PS_FN uint32_t ps_cksum_term(uint32_t s, int x, int y, int bps)
{
  const uint32_t m = (uint32_t)((x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8));
  uint32_t v = (s & 0xff) ^ m;
  if (bps > 1) v += (s >> 8) ^ m;
  return v;
}
// a lane's group of 8 consecutive samples of a row: index -> (row, first sample); gpr = groups per row
HM_PS_FN void ps_group_pos(int gpr, int idx, int *y, int *x0) { *y = idx / gpr; *x0 = (idx - *y * gpr) * 8; }
// the reference's PSNR / MSE expressions (TEncGOP.cpp:2287-2290), evaluated on the host
static inline double ps_psnr(unsigned long long ssd, int size, int bitDepth)
{
  const int maxval = 255 << (bitDepth - 8);
  const double fRefValue = (double)maxval * maxval * size;
  return ssd ? 10.0 * log10(fRefValue / (double)ssd) : 999.99;
}
static inline double ps_mse(unsigned long long ssd, int size) { return (double)ssd / size; }

// ---- CRC (compCRC): 16-bit register, polynomial x^16 + x^12 + x^5 + 1, message bits MSB first, low byte of a sample first.  The register is a
// polynomial remainder: with N message bits, crc = (M(x) x^16 + 0xffff x^(N+16)) mod P, linear over GF(2).  A chunk (a run of samples) with the
// remainder r = chunk(x) x^16 mod P and `after` message bits behind it contributes r x^after mod P; everything combines by XOR. ----
HM_PS_FN uint32_t ps_crc_byte(uint32_t crc, uint32_t b)            // one message byte into the remainder (zero-augmented form)
{
  uint32_t x = ((crc >> 8) ^ b) & 0xff;
  x ^= x >> 4;
  return ((crc << 8) ^ (x << 12) ^ (x << 5) ^ x) & 0xffff;
}
HM_PS_FN uint32_t ps_crc_sample(uint32_t crc, uint32_t s, int bps)
{
  crc = ps_crc_byte(crc, s & 0xff);
  if (bps > 1) crc = ps_crc_byte(crc, (s >> 8) & 0xff);
  return crc;
}
HM_PS_FN uint32_t ps_gf_mul(uint32_t a, uint32_t b)                // carry-less 16 x 16 multiply mod P
{
  uint32_t r = 0;
  for (int i = 0; i < 16; i++) {
    if (b & 1) r ^= a;
    b >>= 1;
    a <<= 1;
    if (a & 0x10000u) a ^= 0x11021u;
  }
  return r;
}
HM_PS_FN uint32_t ps_xpow(uint32_t e)                              // x^e mod P; x has multiplicative order 32,767
{
  e %= 32767u;
  uint32_t r = 1, b = 2;
  while (e) { if (e & 1) r = ps_gf_mul(r, b); b = ps_gf_mul(b, b); e >>= 1; }
  return r;
}
// x^(bits of `samples` samples + extra) mod P, without forming the bit count (a 4K plane has 2^27 bits, larger ones stay exact too)
HM_PS_FN uint32_t ps_xpow_samples(uint32_t samples, int bps, uint32_t extra) { return ps_xpow((samples % 32767u) * (uint32_t)(8 * bps) + extra); }
// chunk k of a plane of wc x hc samples cut into runs of `chunk` samples (a multiple of 8) that never cross a row
struct PsChunk { int32_t y, x0, count; uint32_t after; };          // after: samples of the plane behind the chunk
HM_PS_FN int ps_crc_chunks_per_row(int wc, int chunk) { return (wc + chunk - 1) / chunk; }
HM_PS_FN PsChunk ps_crc_chunk(int wc, int hc, int chunk, int k)
{
  const int cpr = ps_crc_chunks_per_row(wc, chunk);
  PsChunk q;
  q.y = k / cpr; q.x0 = (k - q.y * cpr) * chunk;
  q.count = wc - q.x0 < chunk ? wc - q.x0 : chunk;
  q.after = (uint32_t)wc * (uint32_t)hc - ((uint32_t)q.y * (uint32_t)wc + (uint32_t)q.x0 + (uint32_t)q.count);
  return q;
}
HM_PS_FN uint32_t ps_crc_chunk_term(uint32_t r, uint32_t after, int bps) { return ps_gf_mul(r, ps_xpow_samples(after, bps, 0)); }
HM_PS_FN uint32_t ps_crc_init_term(int wc, int hc, int bps) { return ps_gf_mul(0xffffu, ps_xpow_samples((uint32_t)wc * (uint32_t)hc, bps, 16)); }

// ---- MD5 (RFC 1321) over the plane's bytes: 1 byte per sample up to 8 bits, else 2, low byte first.  The message is handled in units of 4
// samples (a row is a multiple of 4 samples wide, so a unit never crosses a row): 1 message word at 8 bits, 2 above. ----
HM_PS_FN uint32_t ps_rotl(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
HM_PS_FN void ps_md5_init(uint32_t st[4]) { st[0] = 0x67452301u; st[1] = 0xefcdab89u; st[2] = 0x98badcfeu; st[3] = 0x10325476u; }
HM_PS_FN void ps_md5_block(uint32_t st[4], const uint32_t M[16])
{
  const uint32_t K[64] = {
    0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
    0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
    0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
    0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
    0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
    0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
    0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
    0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u };
  const int S[16] = { 7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21 };
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    uint32_t f; int g;
    if (i < 16) { f = (b & c) | (~b & d); g = i; }
    else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
    else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
    else { f = c ^ (b | ~d); g = (7 * i) & 15; }
    const uint32_t t = a + f + K[i] + M[g];
    a = d; d = c; c = b;
    b = b + ps_rotl(t, S[(i >> 4) * 4 + (i & 3)]);
  }
  st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}
// framing of a message of L bytes (L a multiple of 4): the 0x80 byte, zeros, the 64-bit bit length
HM_PS_FN uint32_t ps_md5_blocks(uint64_t L) { return (uint32_t)((L + 8) / 64 + 1); }
HM_PS_FN uint32_t ps_md5_pad_word(uint64_t L, uint64_t w)          // message word w >= L / 4
{
  const uint64_t tw = (uint64_t)ps_md5_blocks(L) * 16;
  if (w == L / 4) return 0x80u;
  if (w == tw - 2) return (uint32_t)(L * 8);
  if (w == tw - 1) return (uint32_t)((L * 8) >> 32);
  return 0;
}
// unit k of block b -> first sample of the unit in raster order of the plane (upb = units per 64-byte block: 16 / bps)
HM_PS_FN uint32_t ps_md5_unit_sample(uint32_t b, int upb, int k) { return (b * (uint32_t)upb + (uint32_t)k) * 4u; }
// the message words of a unit of 4 samples (low 16 bits of each): 1 word with 1 byte per sample, else 2
HM_PS_FN void ps_md5_unit_words(const uint32_t s[4], int bps, uint32_t w[2])
{
  if (bps == 1) { w[0] = (s[0] & 0xff) | ((s[1] & 0xff) << 8) | ((s[2] & 0xff) << 16) | ((s[3] & 0xff) << 24); w[1] = 0; }
  else { w[0] = (s[0] & 0xffff) | ((s[1] & 0xffff) << 16); w[1] = (s[2] & 0xffff) | ((s[3] & 0xffff) << 16); }
}

#if !defined(HM355_HOSTSIM)
// ------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------
#define HM_PS_BLOCK 256
#define HM_PS_GROUPS 4                // groups of 8 samples per lane of hm355_picstat_kernel
#define HM_CRC_CHUNK 64               // samples per lane of hm355_crc_kernel (one 128-byte line of a 16-bit row)

// grid (ceil(groups of the luma plane / (256 * HM_PS_GROUPS)), 1, 3 * n): blockIdx.z = picture * 3 + component.  One 16-byte load per lane and
// picture along the row, 64-bit accumulation, wave reduction, one atomic per workgroup and quantity.
extern "C" __global__ void __launch_bounds__(HM_PS_BLOCK) hm355_picstat_kernel(const Params *P, const PicStatParams *pps, PicStatAcc *acc)
{
  __shared__ unsigned long long redSsd[HM_PS_BLOCK / 64];
  __shared__ uint32_t redSum[HM_PS_BLOCK / 64];
  const int f = (int)blockIdx.z / 3, c = (int)blockIdx.z % 3, cs = c ? 1 : 0;
  const PicStatParams pp = pps[f];
  const int wc = P->width >> cs, hc = P->height >> cs, bps = P->bitDepth > 8 ? 2 : 1;
  const int sw = wc - (pp.padRight >> cs), sh = hc - (pp.padBottom >> cs);       // the SSD's area
  const int gpr = (wc + 7) >> 3, total = gpr * hc, doSum = pp.hashMethod == 3;
  const Pel *org = P->frames[f].org[c], *rec = P->frames[f].rec[c];
  const int stride = P->stride[c];
  unsigned long long ssd = 0; uint32_t sum = 0;
  for (int i = 0; i < HM_PS_GROUPS; i++) {
    const int idx = ((int)blockIdx.x * HM_PS_GROUPS + i) * HM_PS_BLOCK + (int)threadIdx.x;
    if (idx >= total) break;
    int y, x0; ps_group_pos(gpr, idx, &y, &x0);
    const int inSsd = y < sh && x0 < sw;
    if (!inSsd && !doSum) continue;
    alignas(16) Pel r[8], o[8];
    *(uint4 *)r = *(const uint4 *)(rec + (size_t)y * stride + x0);     // the slot's rows are padded to whole CTUs: always readable
    if (inSsd) *(uint4 *)o = *(const uint4 *)(org + (size_t)y * stride + x0);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int x = x0 + j;
      if (inSsd && x < sw) ssd += ps_ssd_term((int)o[j], (int)r[j]);
      if (doSum && x < wc) sum += ps_cksum_term((uint32_t)(uint16_t)r[j], x, y, bps);
    }
  }
  for (int d = 32; d > 0; d >>= 1) { ssd += __shfl_down(ssd, d, 64); sum += __shfl_down(sum, d, 64); }
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { redSsd[wave] = ssd; redSum[wave] = sum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < HM_PS_BLOCK / 64; w++) { ssd += redSsd[w]; sum += redSum[w]; }
    if (ssd) atomicAdd(&acc[f].ssd[c], ssd);
    if (sum) atomicAdd(&acc[f].cksum[c], sum);
  }
}

// grid (ceil(chunks of the luma plane / 256), 1, 3 * n).  Each lane takes the remainder of its own run of `chunk` samples with a zero start
// value and multiplies it by the power of x for its distance to the end of the plane; the workgroup XORs its lanes' terms into the picture's word.
extern "C" __global__ void __launch_bounds__(HM_PS_BLOCK) hm355_crc_kernel(const Params *P, const PicStatParams *pps, PicStatAcc *acc, int chunk)
{
  __shared__ uint32_t red[HM_PS_BLOCK / 64];
  const int f = (int)blockIdx.z / 3, c = (int)blockIdx.z % 3, cs = c ? 1 : 0;
  if (pps[f].hashMethod != 2) return;                              // uniform for the workgroup
  const int wc = P->width >> cs, hc = P->height >> cs, bps = P->bitDepth > 8 ? 2 : 1;
  const int k = (int)blockIdx.x * HM_PS_BLOCK + (int)threadIdx.x;
  uint32_t t = 0;
  if (k < ps_crc_chunks_per_row(wc, chunk) * hc) {
    const PsChunk q = ps_crc_chunk(wc, hc, chunk, k);
    const Pel *row = P->frames[f].rec[c] + (size_t)q.y * P->stride[c] + q.x0;
    uint32_t r = 0;
    for (int x = 0; x < q.count; x += 8) {
      alignas(16) Pel v[8];
      *(uint4 *)v = *(const uint4 *)(row + x);                     // q.x0 is a multiple of 8; the rows are padded to whole CTUs
#pragma unroll
      for (int j = 0; j < 8; j++) if (x + j < q.count) r = ps_crc_sample(r, (uint32_t)(uint16_t)v[j], bps);
    }
    t = ps_crc_chunk_term(r, q.after, bps);
  }
  for (int d = 32; d > 0; d >>= 1) t ^= __shfl_xor(t, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < HM_PS_BLOCK / 64; w++) t ^= red[w];
    if (t) atomicXor(&acc[f].crc[c], t);
  }
}

// MD5 cannot be split inside a plane (every block's 64 steps depend on the block before), so the parallelism is across chains: grid
// (ceil(n / 64), 3), one wavefront per 64 pictures of one component (chains of equal length finish together), lane l runs the chain of picture
// first + l.  Per 64-byte block the wavefront fetches every chain's units of 4 samples (8-byte loads: a unit never crosses a row and is 8-byte
// aligned; consecutive lanes take consecutive units of a chain, and a lane takes the same unit of every block), packs them to message words (8-bit pictures narrow the samples to bytes) and
// hands them to the owning lane through LDS; the loads of block b + 1 are in flight while block b is hashed.  The padding and the 64-bit bit
// length come from ps_md5_pad_word, on the device.
#define HM_MD5_LDS_STRIDE 17          // words per chain in LDS: 16 + 1 keeps the owners' reads free of bank conflicts
template <int BPS> __device__ __forceinline__ void md5_chains(const Params *P, const PicStatParams *pps, PicStatAcc *acc, int n, uint32_t *msg)
{
  constexpr int UPB = 16 / BPS;       // units per block, and the most one lane fetches per block (64 chains)
  const int c = (int)blockIdx.y, cs = c ? 1 : 0, lane = (int)threadIdx.x;
  const int first = (int)blockIdx.x * 64, chains = n - first < 64 ? n - first : 64;
  const int wc = P->width >> cs, hc = P->height >> cs, stride = P->stride[c];
  const uint32_t samples = (uint32_t)wc * (uint32_t)hc;
  const uint64_t L = (uint64_t)samples * BPS;
  const uint32_t nblk = ps_md5_blocks(L);
  const int mine = lane < chains && pps[first + (lane < chains ? lane : 0)].hashMethod == 1;
  uint32_t st[4]; ps_md5_init(st);
  // a lane fetches the same unit k of every block for up to UPB chains (iteration it: chain chBase + it * (64 / UPB)), so the unit's place in
  // the plane is computed once per block and the chains' plane pointers once per launch
  const int k = lane % UPB, chBase = lane / UPB;
  const Pel *base[UPB];
#pragma unroll
  for (int it = 0; it < UPB; it++) { const int ch = chBase + it * (64 / UPB); base[it] = ch < chains ? P->frames[first + ch].rec[c] : (const Pel *)0; }
  uint32_t buf[UPB][BPS];
  auto fetch = [&](uint32_t b) {
    const uint32_t s4 = ps_md5_unit_sample(b, UPB, k);
    if (s4 < samples) {
      const uint32_t y = s4 / (uint32_t)wc, x = s4 - y * (uint32_t)wc;
      const size_t off = (size_t)y * stride + x;
#pragma unroll
      for (int it = 0; it < UPB; it++) {
        if (!base[it]) continue;
        alignas(8) Pel v[4];
        *(uint2 *)v = *(const uint2 *)(base[it] + off);
        const uint32_t s[4] = { (uint32_t)(uint16_t)v[0], (uint32_t)(uint16_t)v[1], (uint32_t)(uint16_t)v[2], (uint32_t)(uint16_t)v[3] };
        uint32_t w[2]; ps_md5_unit_words(s, BPS, w);
#pragma unroll
        for (int j = 0; j < BPS; j++) buf[it][j] = w[j];
      }
    } else {
#pragma unroll
      for (int j = 0; j < BPS; j++) {
        const uint32_t w = ps_md5_pad_word(L, (uint64_t)(s4 / 4) * BPS + j);
#pragma unroll
        for (int it = 0; it < UPB; it++) buf[it][j] = w;
      }
    }
  };
  fetch(0);
  for (uint32_t b = 0; b < nblk; b++) {
#pragma unroll
    for (int it = 0; it < UPB; it++) {
      if (!base[it]) continue;
      const int ch = chBase + it * (64 / UPB);
#pragma unroll
      for (int j = 0; j < BPS; j++) msg[ch * HM_MD5_LDS_STRIDE + k * BPS + j] = buf[it][j];
    }
    __syncthreads();
    uint32_t M[16];
#pragma unroll
    for (int k = 0; k < 16; k++) M[k] = msg[lane * HM_MD5_LDS_STRIDE + k];
    __syncthreads();
    if (b + 1 < nblk) fetch(b + 1);
    if (mine) ps_md5_block(st, M);
  }
  if (mine) for (int k = 0; k < 4; k++) acc[first + lane].md5[c][k] = st[k];
}
extern "C" __global__ void __launch_bounds__(64) hm355_md5_kernel(const Params *P, const PicStatParams *pps, PicStatAcc *acc, int n)
{
  __shared__ uint32_t msg[64 * HM_MD5_LDS_STRIDE];
  if (P->bitDepth > 8) md5_chains<2>(P, pps, acc, n, msg); else md5_chains<1>(P, pps, acc, n, msg);
}
#endif
