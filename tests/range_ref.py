"""numpy reference of the range probe (csrc/range_probe.hip): pair16 decoder and the four words of a record, from stored bits."""
import numpy as np

F32, F16X2, BF16X2 = 0, 1, 2


def decode_pair16(words, storage):
    """words (..., C) uint32, C % 8 == 0: the pair16 row layout of csrc/hgemm.h - each group of 8 channels is 16 bytes of hi halves
    followed by 16 bytes of lo halves.  Returns (hi bits, lo bits, hi fp32, lo fp32), each (..., C)."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    shp = words.shape
    g = shp[-1] // 8
    halves = words.view(np.uint16).reshape(*shp[:-1], g, 2, 8)
    hb = np.ascontiguousarray(halves[..., 0, :]).reshape(shp)
    lb = np.ascontiguousarray(halves[..., 1, :]).reshape(shp)
    if storage == F16X2:
        return hb, lb, hb.view(np.float16).astype(np.float32), lb.view(np.float16).astype(np.float32)
    return hb, lb, (hb.astype(np.uint32) << 16).view(np.float32), (lb.astype(np.uint32) << 16).view(np.float32)


def encode_pair16(hb, lb):
    """Inverse of the layout: hi / lo bits (..., C) uint16 -> words (..., C) uint32."""
    shp = hb.shape
    g = shp[-1] // 8
    halves = np.stack([hb.reshape(*shp[:-1], g, 8), lb.reshape(*shp[:-1], g, 8)], axis=-2).astype(np.uint16)
    return np.ascontiguousarray(halves).reshape(*shp[:-1], g * 16).view(np.uint32).reshape(shp)


def probe_reference(words, storage, rows=None, c_off=0, c=None):
    """(peak bits uint32, saturated, nonfinite, elements) of rows [0, rows) x channels [c_off, c_off + c) of words (R, stride) uint32."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    rows = words.shape[0] if rows is None else min(int(rows), words.shape[0])
    c = words.shape[1] - c_off if c is None else c
    w = np.ascontiguousarray(words[:rows, c_off:c_off + c])
    if w.size == 0:
        return 0, 0, 0, rows * c
    with np.errstate(all='ignore'):
        if storage == F32:
            v = w.view(np.float32)
            bad = ~np.isfinite(v)
            sat = 0
        else:
            hb, lb, hi, lo = decode_pair16(w, storage)
            v = hi + lo                                     # np.float32(hi) + np.float32(lo): one fp32 addition, as M::join
            bad = ~np.isfinite(hi) | ~np.isfinite(lo)
            sat = int(((hb & 0x7FFF) == 0x7BFF).sum()) if storage == F16X2 else 0
        mag = np.abs(v).astype(np.float32).view(np.uint32)
    peak = int(mag[~bad].max()) if (~bad).any() else 0
    return peak, sat, int(bad.sum()), rows * c
