"""The packed row format of the 4-bit fast-scan PQ index (include/mevi_hip_pqfs.h) in numpy, for the tests of mevi_pq4_pack and
mevi_pqfs_scan_topk_f32.  The reference of the scan itself is tests/ivfpq_cases.py: adc_expected with K = 16 over the UNPACKED
codes; nothing here is a tolerance."""
import numpy as np


def pack(codes):
    """u8 [n, m] -> u8 [n, m / 2]: byte t = (code 2t & 15) | (code 2t + 1 & 15) << 4."""
    codes = np.asarray(codes, np.uint8)
    assert codes.ndim == 2 and codes.shape[1] % 2 == 0
    return ((codes[:, 0::2] & 15) | ((codes[:, 1::2] & 15) << 4)).astype(np.uint8)


def unpack(packed):
    """u8 [n, m / 2] -> u8 [n, m]: code 2t = low nibble of byte t, code 2t + 1 = its high nibble."""
    packed = np.asarray(packed, np.uint8)
    out = np.empty((packed.shape[0], 2 * packed.shape[1]), np.uint8)
    out[:, 0::2] = packed & 15
    out[:, 1::2] = packed >> 4
    return out


def unpack_swapped(packed):
    """The WRONG reading (code 2t from the high nibble): what a scan with the nibbles the other way round would score."""
    packed = np.asarray(packed, np.uint8)
    out = np.empty((packed.shape[0], 2 * packed.shape[1]), np.uint8)
    out[:, 0::2] = packed >> 4
    out[:, 1::2] = packed & 15
    return out
