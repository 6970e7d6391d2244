"""numpy restatements behind tests/test_rng_host.py and tests/test_gpu_input_rng_adam.py — TEST INFRASTRUCTURE ONLY.

  * Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library publishes the
    known-answer vectors tests/test_rng_host.py pins it on) and the library's mapping on top of it (csrc/misc.hip):
    counter words (ctr lo, ctr hi, 0x243F6A88, 0x85A308D3), key (seed lo, seed hi), one counter per group of four outputs;
  * the two maps from a 32-bit word to a float: vcg_rand_uniform's (word >> 8) * 2^-24 in [0, 1), and u01 of the normal draws,
    ((float)(word >> 8) + 0.5f) * 2^-24 IN FP32 — the addition rounds to nearest even once word >> 8 >= 2^23, so the top word
    gives u == 1.0f exactly; that rounding is part of the stream's definition, Box-Muller on top of it is done in float64;
  * a float32 restatement of input_oracle.resample (same formulas, every intermediate rounded to fp32, the tap centre included)
    and the per-element rounding bound of a double sum the resample test builds its tolerance from.
"""
import numpy as np

import input_oracle as io

# ---------------------------------------------------------------------------------------------------------------- Philox
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
LIB_C2, LIB_C3 = 0x243F6A88, 0x85A308D3
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: (..., 4), key: (..., 2) arrays of 32-bit words -> (..., 4) uint32"""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> s32) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + np.uint64(PHILOX_W0)) & MASK32, (k[1] + np.uint64(PHILOX_W1)) & MASK32]
    return np.stack(c, -1).astype(np.uint32)


def lib_words(seed, offset, nquads):
    """The (nquads, 4) words the library draws at counters offset .. offset + nquads - 1 (mod 2^64) of stream `seed`."""
    ctr = (np.arange(nquads, dtype=np.uint64) + np.uint64(offset & 0xFFFFFFFFFFFFFFFF))     # uint64 addition wraps
    counter = np.stack([ctr & MASK32, ctr >> np.uint64(32), np.full_like(ctr, LIB_C2), np.full_like(ctr, LIB_C3)], -1)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64)
    return philox4x32_10(counter, np.broadcast_to(key, (nquads, 2)))


def uniform_of(words):
    """vcg_rand_uniform: exact in fp32 (24 bits times a power of two)"""
    return (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def u01_of(words):
    """u01 of the normal draws, with its fp32 addition"""
    return ((words >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def randn_of(words):
    """(nquads, 4) words -> (nquads, 4) float64: Box-Muller on (word 0, word 1) and (word 2, word 3), cos first"""
    u = u01_of(words).astype(np.float64)
    out = np.empty(words.shape, np.float64)
    for a in (0, 2):
        r = np.sqrt(-2.0 * np.log(u[..., a]))
        th = 2.0 * np.pi * u[..., a + 1]
        out[..., a], out[..., a + 1] = r * np.cos(th), r * np.sin(th)
    return out


# ---------------------------------------------------------------------------------------------------------------- resample
def _weights(box_len, S, filt, dtype):
    """input_oracle.resample_weights in crop coordinates with every intermediate of type `dtype`: [(first tap, normalised
    weights, sum of the raw weights)]"""
    f = dtype
    fn, support = io.FILTERS[filt]
    scale = f(box_len) / f(S)
    fscale = scale if scale > f(1) else f(1)
    sup = f(support) * fscale
    out = []
    for o in range(S):
        center = (f(o) + f(0.5)) * scale
        xmin = max(int(center - sup + f(0.5)), 0)
        xmax = min(int(center + sup + f(0.5)), box_len)
        xs = np.arange(xmin, xmax).astype(dtype)
        arg = ((xs - center + f(0.5)) / fscale).astype(dtype)
        x = np.abs(arg)
        if filt == 0:                                        # input_oracle._bicubic, term by term in `dtype`
            a = f(-0.5)
            w = np.where(x < 1, ((a + f(2)) * x - (a + f(3))) * x * x + f(1), np.where(x < 2, (((x - f(5)) * x + f(8)) * x - f(4)) * a, f(0)))
        else:
            w = np.where(x < 1, f(1) - x, f(0))
        w = w.astype(dtype)
        s = dtype(0)
        for v in w:                                          # a running sum in `dtype`, not numpy's pairwise one
            s = dtype(s + v)
        out.append((xmin, (w / s).astype(dtype) if s != 0 else w, s))
    return out


def _apply(crop, wx, wy, dtype):
    """the two separable passes of input_oracle.resample (horizontal, then vertical), accumulated tap by tap in `dtype`"""
    S = len(wx)
    tmp = np.zeros((crop.shape[0], S, 3), dtype)
    for o, (first, w, _) in enumerate(wx):
        acc = np.zeros((crop.shape[0], 3), dtype)
        for k, wk in enumerate(w):
            acc = (acc + wk * crop[:, first + k]).astype(dtype)
        tmp[:, o] = acc
    out = np.zeros((S, S, 3), dtype)
    for o, (first, w, _) in enumerate(wy):
        acc = np.zeros((S, 3), dtype)
        for k, wk in enumerate(w):
            acc = (acc + wk * tmp[first + k]).astype(dtype)
        out[o] = acc
    return out


def _crop(src, box, flip_h, flip_v):
    img = src
    if flip_h:
        img = img[:, ::-1]
    if flip_v:
        img = img[::-1]
    y0, x0, h, w = box
    return img[y0:y0 + h, x0:x0 + w]


def resample_f32(src, box, S, flip_h=False, flip_v=False, filt=0):
    """input_oracle.resample with float32 for every intermediate: weights (tap centre, filter argument, normalisation), both
    passes, the final division by 255."""
    f = np.float32
    unit = f(255.0) if src.dtype == np.uint8 else f(1.0)
    crop = _crop(src, box, flip_h, flip_v).astype(f)
    return (_apply(crop, _weights(box[3], S, filt, f), _weights(box[2], S, filt, f), f) / unit).astype(f)


def resample_abs(src, box, S, flip_h=False, flip_v=False, filt=0):
    """sum |w_y| |w_x| |v| / (|sum w_y| |sum w_x|) per output element, in float64 and in units of the output: what one rounding
    of relative size U per term of the double sum can add up to."""
    d = np.float64
    unit = 255.0 if src.dtype == np.uint8 else 1.0
    crop = np.abs(_crop(src, box, flip_h, flip_v).astype(d))
    wx = [(a, np.abs(w), s) for a, w, s in _weights(box[3], S, filt, d)]
    wy = [(a, np.abs(w), s) for a, w, s in _weights(box[2], S, filt, d)]
    return _apply(crop, wx, wy, d) / unit


def resample_tolerance(src, box, S, flip_h, flip_v, filt, ref=None):
    """(per-element tolerance, E) of the unquantised resample: 4 E + 8 U sum|w_y||w_x||v| / (|sum w_y||sum w_x|), with E the largest
    |fp32 restatement - float64 oracle| over this image and U = 2^-24."""
    if ref is None:
        ref = io.resample(src, box, S, flip_h, flip_v, filt)
    E = float(np.abs(resample_f32(src, box, S, flip_h, flip_v, filt).astype(np.float64) - ref).max())
    return 4.0 * E + 8.0 * 2.0 ** -24 * resample_abs(src, box, S, flip_h, flip_v, filt), E


def quantised_disagreement(src, box, S, flip_h, flip_v, filt):
    """share of the output values on which the fp32 restatement and the float64 oracle pick different uint8 levels"""
    a = io.quantize_u8(resample_f32(src, box, S, flip_h, flip_v, filt))
    b = io.quantize_u8(io.resample(src, box, S, flip_h, flip_v, filt))
    return float((a != b).mean())
