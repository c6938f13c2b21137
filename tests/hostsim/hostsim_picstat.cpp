// CPU twin of hm-16.2_amd/csrc/hm355_picstat.h: the header's arithmetic (compiled under HM355_HOSTSIM, no HIP headers) driven by plain loops that
// walk the planes exactly as the kernels partition them -- groups of 8 samples per lane of hm355_picstat_kernel, runs of `chunk` samples per lane of
// hm355_crc_kernel, units of 4 samples per fetching lane and 64-byte blocks per chain of hm355_md5_kernel -- forwards or backwards.
//   hostsim_picstat <file> <chunk> <reverse>
// file: int32 width, height, bitDepth, padRight, padBottom, hashMethod; the original Y, Cb, Cr planes (uint16, tightly packed), the reconstruction
// the same way.  Prints "ssd a b c", "psnr <the log line's piece>", "mse a b c" (hex floats) and "digest <digestToString>".
#define HM355_HOSTSIM 1
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../hm-16.2_amd/csrc/hm355_types.h"
#include "../../hm-16.2_amd/csrc/hm355_picstat.h"

#define BLOCK 256
#define GROUPS 4

struct Plane { std::vector<Pel> v; int stride; };
static Plane slot_plane(const uint16_t *src, int wc, int hc, int stride, int rows)   // the slot's layout: rows padded to whole CTUs, the padding holds junk
{
  Plane p; p.stride = stride; p.v.assign((size_t)stride * rows, (Pel)0x5a5a);
  for (int y = 0; y < hc; y++) for (int x = 0; x < wc; x++) p.v[(size_t)y * stride + x] = (Pel)src[(size_t)y * wc + x];
  return p;
}

int main(int argc, char **argv)
{
  if (argc < 4) { fprintf(stderr, "usage: hostsim_picstat file chunk reverse\n"); return 2; }
  FILE *fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  const int chunk = atoi(argv[2]), reverse = atoi(argv[3]);
  if (chunk < 8 || (chunk & 7)) { fprintf(stderr, "chunk must be a multiple of 8\n"); return 2; }
  int32_t hd[6];
  if (fread(hd, 4, 6, fp) != 6) return 2;
  const int width = hd[0], height = hd[1], bitDepth = hd[2], padRight = hd[3], padBottom = hd[4], method = hd[5];
  const int wCtu = (width + 63) / 64, hCtu = (height + 63) / 64, bps = bitDepth > 8 ? 2 : 1;
  Plane org[3], rec[3];
  for (int pic = 0; pic < 2; pic++) for (int c = 0; c < 3; c++) {
    const int wc = width >> (c ? 1 : 0), hc = height >> (c ? 1 : 0);
    std::vector<uint16_t> t((size_t)wc * hc);
    if (fread(t.data(), 2, t.size(), fp) != t.size()) return 2;
    (pic ? rec : org)[c] = slot_plane(t.data(), wc, hc, wCtu * (c ? 32 : 64), hCtu * (c ? 32 : 64));
  }
  fclose(fp);
  PicStatAcc acc; memset(&acc, 0, sizeof(acc));
  for (int c = 0; c < 3; c++) {
    const int cs = c ? 1 : 0, wc = width >> cs, hc = height >> cs, stride = org[c].stride;
    // ---- hm355_picstat_kernel ----
    {
      const int sw = wc - (padRight >> cs), sh = hc - (padBottom >> cs), gpr = (wc + 7) >> 3, total = gpr * hc, doSum = method == 3;
      const int lumaGroups = ((width + 7) / 8) * height, grid = (lumaGroups + BLOCK * GROUPS - 1) / (BLOCK * GROUPS);
      for (int b0 = 0; b0 < grid; b0++) {
        const int bx = reverse ? grid - 1 - b0 : b0;
        unsigned long long wgSsd = 0; uint32_t wgSum = 0;
        for (int t0 = 0; t0 < BLOCK; t0++) {
          const int tid = reverse ? BLOCK - 1 - t0 : t0;
          unsigned long long ssd = 0; uint32_t sum = 0;
          for (int i = 0; i < GROUPS; i++) {
            const int idx = (bx * GROUPS + i) * BLOCK + tid;
            if (idx >= total) break;
            int y, x0; ps_group_pos(gpr, idx, &y, &x0);
            const int inSsd = y < sh && x0 < sw;
            if (!inSsd && !doSum) continue;
            const Pel *r = &rec[c].v[(size_t)y * stride + x0], *o = &org[c].v[(size_t)y * stride + x0];
            for (int j = 0; j < 8; j++) {
              const int x = x0 + j;
              if (inSsd && x < sw) ssd += ps_ssd_term((int)o[j], (int)r[j]);
              if (doSum && x < wc) sum += ps_cksum_term((uint32_t)(uint16_t)r[j], x, y, bps);
            }
          }
          wgSsd += ssd; wgSum += sum;
        }
        acc.ssd[c] += wgSsd; acc.cksum[c] += wgSum;
      }
    }
    // ---- hm355_crc_kernel ----
    if (method == 2) {
      const int chunks = ps_crc_chunks_per_row(wc, chunk) * hc;
      for (int k0 = 0; k0 < chunks; k0++) {
        const int k = reverse ? chunks - 1 - k0 : k0;
        const PsChunk q = ps_crc_chunk(wc, hc, chunk, k);
        const Pel *row = &rec[c].v[(size_t)q.y * stride + q.x0];
        uint32_t r = 0;
        for (int x = 0; x < q.count; x += 8)
          for (int j = 0; j < 8; j++) if (x + j < q.count) r = ps_crc_sample(r, (uint32_t)(uint16_t)row[x + j], bps);
        acc.crc[c] ^= ps_crc_chunk_term(r, q.after, bps);
      }
    }
    // ---- hm355_md5_kernel: one chain ----
    if (method == 1) {
      const int upb = 16 / bps;
      const uint32_t samples = (uint32_t)wc * (uint32_t)hc;
      const uint64_t L = (uint64_t)samples * bps;
      const uint32_t nblk = ps_md5_blocks(L);
      uint32_t st[4]; ps_md5_init(st);
      for (uint32_t b = 0; b < nblk; b++) {
        uint32_t msg[17];
        for (int u0 = 0; u0 < upb; u0++) {           // the fetching lanes
          const int k = reverse ? upb - 1 - u0 : u0;
          const uint32_t s4 = ps_md5_unit_sample(b, upb, k);
          uint32_t w[2];
          if (s4 < samples) {
            const uint32_t y = s4 / (uint32_t)wc, x = s4 - y * (uint32_t)wc;
            const Pel *v = &rec[c].v[(size_t)y * stride + x];
            const uint32_t s[4] = { (uint32_t)(uint16_t)v[0], (uint32_t)(uint16_t)v[1], (uint32_t)(uint16_t)v[2], (uint32_t)(uint16_t)v[3] };
            ps_md5_unit_words(s, bps, w);
          } else for (int j = 0; j < bps; j++) w[j] = ps_md5_pad_word(L, (uint64_t)(s4 / 4) * bps + j);
          for (int j = 0; j < bps; j++) msg[k * bps + j] = w[j];
        }
        ps_md5_block(st, msg);
      }
      for (int k = 0; k < 4; k++) acc.md5[c][k] = st[k];
    }
  }
  // ---- the host side of hm355_picture_stats_run ----
  double psnr[3], mse[3];
  printf("ssd");
  for (int c = 0; c < 3; c++) {
    const int cs = c ? 1 : 0, size = ((width >> cs) - (padRight >> cs)) * ((height >> cs) - (padBottom >> cs));
    psnr[c] = ps_psnr(acc.ssd[c], size, bitDepth); mse[c] = ps_mse(acc.ssd[c], size);
    printf(" %llu", acc.ssd[c]);
  }
  printf("\npsnr [Y %6.4lf dB    U %6.4lf dB    V %6.4lf dB]\n", psnr[0], psnr[1], psnr[2]);
  printf("mse %a %a %a\n", mse[0], mse[1], mse[2]);
  printf("digest ");
  const int len = method == 1 ? 16 : (method == 2 ? 2 : (method == 3 ? 4 : 0));
  for (int c = 0; c < 3; c++) {
    const int cs = c ? 1 : 0;
    uint8_t d[16];
    if (method == 1) for (int i = 0; i < 16; i++) d[i] = (uint8_t)(acc.md5[c][i >> 2] >> (8 * (i & 3)));
    else if (method == 2) { const uint32_t v = acc.crc[c] ^ ps_crc_init_term(width >> cs, height >> cs, bps); d[0] = (uint8_t)(v >> 8); d[1] = (uint8_t)v; }
    else if (method == 3) for (int i = 0; i < 4; i++) d[i] = (uint8_t)(acc.cksum[c] >> (24 - 8 * i));
    if (c && len) printf(",");
    for (int i = 0; i < len; i++) printf("%02x", d[i]);
  }
  printf("\n");
  return 0;
}
