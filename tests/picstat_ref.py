"""numpy / hashlib restatement of what the reference computes on a finished picture: the SSD / PSNR / MSE of TEncGOP::xCalculateAddPSNR and the
decoded picture hashes of TComPicYuvMD5.cpp (calcMD5, calcCRC, calcChecksum).  tests/test_picture_stats_host.py pins it by the reference's own
log lines (tests/golden/pichash_*.npz), so that it can serve as the oracle on fresh inputs; it is fast enough for 4K planes."""
import binascii
import hashlib
import math

import numpy as np

DIGEST_LEN = {0: 0, 1: 16, 2: 2, 3: 4}


def plane_bytes(plane, bit_depth):
    """the byte string the hashes run over: rows in raster order, 1 byte per sample up to 8 bits (the low byte), else 2, low byte first"""
    p = np.ascontiguousarray(plane, np.uint16)
    return (p & 0xff).astype(np.uint8).tobytes() if bit_depth <= 8 else p.astype("<u2").tobytes()


def md5(plane, bit_depth):
    return hashlib.md5(plane_bytes(plane, bit_depth)).digest()


def crc(plane, bit_depth):
    """compCRC: 0x1D0F is the initial value 0xffff advanced by 16 zero bits, which turns the reference's register into the zero-augmented form"""
    v = binascii.crc_hqx(plane_bytes(plane, bit_depth), 0x1D0F)
    return bytes([v >> 8, v & 0xff])


def crc_bitwise(plane, bit_depth):
    """compCRC bit by bit (small planes only)"""
    c = 0xffff
    for b in plane_bytes(plane, bit_depth):
        for i in range(8):
            msb = (c >> 15) & 1
            c = (((c << 1) + ((b >> (7 - i)) & 1)) & 0xffff) ^ (msb * 0x1021)
    for i in range(16):
        msb = (c >> 15) & 1
        c = ((c << 1) & 0xffff) ^ (msb * 0x1021)
    return bytes([c >> 8, c & 0xff])


def checksum(plane, bit_depth):
    p = np.ascontiguousarray(plane, np.uint16).astype(np.uint64)
    h, w = p.shape
    x, y = np.arange(w, dtype=np.uint64)[None, :], np.arange(h, dtype=np.uint64)[:, None]
    mask = (x & 0xff) ^ (y & 0xff) ^ (x >> 8) ^ (y >> 8)
    s = int(((p & 0xff) ^ mask).sum(dtype=np.uint64))
    if bit_depth > 8:
        s += int(((p >> 8) ^ mask).sum(dtype=np.uint64))
    return (s & 0xffffffff).to_bytes(4, "big")


def ssd(org, rec, pad_right=0, pad_bottom=0, chroma=False):
    h, w = org.shape
    w -= pad_right >> (1 if chroma else 0); h -= pad_bottom >> (1 if chroma else 0)
    d = org[:h, :w].astype(np.int64) - rec[:h, :w].astype(np.int64)
    return int((d * d).sum(dtype=np.int64)), w * h


def psnr(ssd_value, size, bit_depth):
    maxval = 255 << (bit_depth - 8)
    return 10.0 * math.log10(float(maxval) * maxval * size / float(ssd_value)) if ssd_value else 999.99


def psnr_string(values):
    return " [Y %6.4f dB    U %6.4f dB    V %6.4f dB]" % tuple(values)


def picture_stats(org, rec, bit_depth, hash_method, pad_right=0, pad_bottom=0):
    """-> dict(ssd, psnr, mse, digest (3 byte strings), digest_string, psnr_string) of one 4:2:0 picture (three planes each)"""
    ssds, sizes = zip(*[ssd(org[k], rec[k], pad_right, pad_bottom, k > 0) for k in range(3)])
    fn = {0: lambda p, b: b"", 1: md5, 2: crc, 3: checksum}[hash_method]
    digest = [fn(rec[k], bit_depth) for k in range(3)]
    ps = tuple(psnr(s, n, bit_depth) for s, n in zip(ssds, sizes))
    return dict(ssd=tuple(ssds), psnr=ps, mse=tuple(float(s) / n for s, n in zip(ssds, sizes)), digest=digest,
                digest_string=",".join(d.hex() for d in digest) if hash_method else "", psnr_string=psnr_string(ps))
