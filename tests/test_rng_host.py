"""What tests/test_gpu_input_rng_adam.py relies on and a CPU can pin:

  * the numpy Philox4x32-10 (oracle/device_oracle.py) against the three known-answer vectors the Random123 library publishes, and
    the library's counter / key mapping on top of it;
  * the two counters of stream 0x5EED5EED whose third word maps to the two ends of u01 (found once by a vectorised search over
    the first 2^25 counters; the words are re-derived here);
  * the resample cases of the GPU module (they are defined here so that both modules use the same ones) and the condition under
    which its quantised check is meaningful: on every input, the fp32 restatement of the oracle and the float64 oracle pick
    different uint8 levels on at most 0.5 % of the values;
  * the three places of csrc/input.hip that assemble a 64-bit offset from two int32 words.  The arena BYTE offset's high word is
    exercised on the device (a 4 GiB arena); a float-buffer PIXEL offset >= 2^32 would need a 64 GiB buffer, so those two are read
    here instead.
"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import device_oracle as do  # noqa: E402
import input_oracle as io  # noqa: E402

from test_input_pipeline import CASES as OLD_CASES  # noqa: E402

# ------------------------------------------------------------------------------------------------------------------ Philox
KNOWN_ANSWERS = [   # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
END_SEED = 0x5EED5EED                      # ops._RNG's default seed
END_ONES = (1279085, 2, 0xFFFFFF66)        # counter, word index, word: top 24 bits all ones  -> u01 == 1.0f
END_ZEROS = (21291187, 2, 0x00000074)      # top 24 bits all zero -> u01 == 2^-25


def test_philox_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = do.philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    # vectorised over a leading axis: the same rows
    got = do.philox4x32_10(np.array([k[0] for k in KNOWN_ANSWERS], np.uint64), np.array([k[1] for k in KNOWN_ANSWERS], np.uint64))
    assert got.dtype == np.uint32 and [tuple(int(x) for x in r) for r in got] == [k[2] for k in KNOWN_ANSWERS]


def test_library_mapping_of_seed_and_offset():
    """counter words = (ctr lo, ctr hi, 0x243F6A88, 0x85A308D3), key = (seed lo, seed hi), ctr = offset + quad (mod 2^64)"""
    seed, off = 0xA4093822299F31D0, (1 << 32) - 2
    w = do.lib_words(seed, off, 4)
    for q in range(4):
        c = off + q
        want = do.philox4x32_10(np.array([c & 0xFFFFFFFF, c >> 32, 0x243F6A88, 0x85A308D3], np.uint64),
                                np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
        assert np.array_equal(w[q], want)
    assert not np.array_equal(w[1], w[2])                                     # the carry into the high word changes the draw ...
    assert not np.array_equal(w[2], do.lib_words(seed, 0, 1)[0])              # ... and is not the counter wrapped to 32 bits
    assert not np.array_equal(do.lib_words(seed, 5, 1), do.lib_words(seed & 0xFFFFFFFF, 5, 1))     # the seed's high word is used
    assert np.array_equal(do.lib_words(seed, (1 << 64) - 1, 2)[1], do.lib_words(seed, 0, 1)[0])    # 64-bit wrap


def test_end_words_of_u01():
    for (ctr, col, word), u in ((END_ONES, 1.0), (END_ZEROS, 2.0 ** -25)):
        w = do.lib_words(END_SEED, ctr, 1)[0]
        assert int(w[col]) == word and col in (0, 2)
        assert do.u01_of(w)[col] == np.float32(u)
    assert END_ONES[2] >> 8 == 0xFFFFFF and END_ZEROS[2] >> 8 == 0
    r = do.randn_of(do.lib_words(END_SEED, END_ONES[0], 1))[0]
    assert r[2] == 0.0 and r[3] == 0.0                                        # u == 1: radius 0
    r = do.randn_of(do.lib_words(END_SEED, END_ZEROS[0], 1))[0]
    assert abs(np.hypot(r[2], r[3]) - np.sqrt(2 * np.log(2.0 ** 25))) < 1e-12  # ~5.887, the longest draw the stream can make
    # the uniform map stays below 1 on the same word
    assert do.uniform_of(np.array([END_ONES[2]], np.uint32))[0] == np.float32(1.0 - 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------------ resample cases
def noise_ramp(seed, h, w):
    """white noise plus a ramp in x and y: nothing a wrong flip or a transposed axis could cancel against"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = np.stack([60 * xx / max(w - 1, 1) + 30 * yy / max(h - 1, 1), 80 * yy / max(h - 1, 1), 50 * xx / max(w - 1, 1) + 10], -1)
    return np.clip(rng.rand(h, w, 3) * 150 + ramp, 0, 255).astype(np.uint8)


def _single_cases():
    """(name, H, W, S, box (y0, x0, h, w), flip_h, flip_v, filter); the source is noise_ramp(crc of the name, H, W)"""
    out = []
    H, W, b = 90, 120, 60
    boxes = {"top": (0, 13, b, b), "left": (11, 0, b, b), "bottom": (H - b, 17, b, b), "right": (9, W - b, b, b)}
    for fh in (0, 1):
        for fv in (0, 1):
            for side, box in boxes.items():
                out.append((f"flip{fh}{fv}-{side}", H, W, 37, box, fh, fv, 0))
    out.append(("whole-frame-bicubic", H, W, 37, (0, 0, H, W), 0, 0, 0))
    out.append(("whole-frame-bilinear-flipped", H, W, 37, (0, 0, H, W), 1, 1, 1))
    for filt in (0, 1):
        for bh, bw in ((1, 1), (2, 2), (3, 3), (1, 40)):                      # every tap range clipped to the crop on both sides
            out.append((f"box{bh}x{bw}-f{filt}", 50, 70, 37, (21, 17, bh, bw), filt, 1 - filt, filt))
    out.append(("shrink8", 600, 700, 64, (50, 100, 512, 512), 1, 0, 0))
    out.append(("shrink16", 1100, 1200, 64, (40, 90, 1024, 1024), 0, 1, 0))
    out.append(("shrink47", 2000, 3000, 64, (0, 0, 2000, 3000), 0, 0, 0))     # 3000 x 2000 frame: 47x in x, 31x in y, 188 taps
    out.append(("upsample8", 80, 90, 256, (20, 30, 32, 32), 1, 1, 0))
    out.append(("resize-1024x768-bilinear", 768, 1024, 256, (0, 0, 768, 1024), 0, 0, 1))   # the hypersim frame, Resize((S, S))
    out.append(("hypersim-crop-bicubic", 768, 1024, 100, (130, 401, 523, 523), 1, 0, 0))   # fp32 tap centres up to 523
    out.append(("S1", 40, 50, 1, (5, 7, 20, 30), 0, 1, 0))
    out.append(("S1-bilinear", 40, 50, 1, (5, 7, 20, 30), 1, 0, 1))
    out.append(("S100", 130, 110, 100, (20, 10, 77, 77), 1, 1, 0))
    return out


SINGLE_CASES = _single_cases()
OLD_SINGLE = [(f"old{k}", c[0], c[1], c[2], c[3], int(c[4]), int(c[5]), c[6]) for k, c in enumerate(OLD_CASES)]


def case_source(case):
    import zlib
    return noise_ramp(zlib.crc32(case[0].encode()) & 0x7FFFFFFF, case[1], case[2])


def old_case_sources():
    """the six cases of test_input_pipeline.py with the white-noise sources that test draws for them"""
    rng = np.random.RandomState(7)
    srcs = {}
    for S in (64, 96, 256):
        for k, c in enumerate(OLD_CASES):
            if c[2] == S:
                srcs[k] = (rng.rand(c[0], c[1], 3) * 255).astype(np.uint8)
    return [srcs[k] for k in range(len(OLD_CASES))]


def batch_cases(seed, N, lo, hi):
    """N different images with drawn sizes in [lo, hi], boxes, flips and filters: [(src, box, flip_h, flip_v, filter)]"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(N):
        h, w = int(rng.randint(lo, hi + 1)), int(rng.randint(lo, hi + 1))
        bh, bw = int(rng.randint(4, h + 1)), int(rng.randint(4, w + 1))
        box = (int(rng.randint(0, h - bh + 1)), int(rng.randint(0, w - bw + 1)), bh, bw)
        out.append((noise_ramp(seed * 1000 + k, h, w), box, int(rng.randint(2)), int(rng.randint(2)), int(rng.randint(2))))
    return out


MIX_N, MIX_S = 17, 37
MIX_FLOAT = (2, 5, 11, 16)               # samples of the N = 17 launch that are read from the float4 buffer
MIX_JITTER = {2: (1.0, 1.1, 0.9, 1.15, 0.05, 1 + 4 * 0 + 16 * 3 + 64 * 2), 5: None, 11: (1.0, 0.8, 1.2, 0.7, -0.08, 3 + 4 * 2 + 16 * 1 + 64 * 0),
              16: None}                  # None: the frame's jitter is disabled (it holds level / 255)
BIG_N, BIG_S = 65, 256                   # 65 x 256 x 256 outputs > 16384 blocks x 256 threads: the grid-stride loop runs


def order_of(code):
    return tuple((int(code) >> (2 * q)) & 3 for q in range(4))


def mix_cases():
    """[(src as the resample reads it, box, fh, fv, filter, quantise, uint8 frame)]: float sources are what vcg_input_prejitter
    leaves for the frame, i.e. the (jittered) uint8 levels / 255 in fp32"""
    out = []
    for k, (src, box, fh, fv, filt) in enumerate(batch_cases(31, MIX_N, 30, 140)):
        seen = src
        if k in MIX_FLOAT:
            j = MIX_JITTER[k]
            lv = src if j is None else io.color_jitter_pil(src, *[float(np.float32(v)) for v in j[1:5]], order_of(j[5]))
            seen = lv.astype(np.float32) / np.float32(255.0)
        out.append((seen, box, fh, fv, filt, k % 2, src))
    return out


def _disagreement(src, box, S, fh, fv, filt):
    return do.quantised_disagreement(src, box, S, bool(fh), bool(fv), filt)


@pytest.mark.parametrize("case", SINGLE_CASES + OLD_SINGLE, ids=[c[0] for c in SINGLE_CASES + OLD_SINGLE])
def test_resample_inputs_meet_the_quantised_checks_condition(case):
    src = old_case_sources()[int(case[0][3:])] if case[0].startswith("old") else case_source(case)
    _, H, W, S, box, fh, fv, filt = case
    assert src.shape == (H, W, 3) and box[0] + box[2] <= H and box[1] + box[3] <= W and min(box[2:]) >= 1
    bad = _disagreement(src, box, S, fh, fv, filt)
    n = S * S * 3
    assert bad <= 0.005 if n >= 4096 else bad * n <= 1, (case[0], bad)
    # the fp32 restatement is a restatement: a filter argument near the tap centre c carries U c, and the weights have slope ~1
    tol, E = do.resample_tolerance(src, box, S, bool(fh), bool(fv), filt)
    assert E <= 4 * 2.0 ** -24 * max(box[2], box[3], 16) and tol.shape == (S, S, 3) and (tol > 0).all(), (case[0], E)


def test_resample_batches_meet_the_quantised_checks_condition():
    for src, box, fh, fv, filt, _, _ in mix_cases():
        assert _disagreement(src, box, MIX_S, fh, fv, filt) <= 0.005
    worst = max(_disagreement(src, box, BIG_S, fh, fv, filt) for src, box, fh, fv, filt in batch_cases(32, BIG_N, 24, 60))
    assert worst <= 0.005, worst


def test_fp32_restatement_is_not_the_float64_oracle():
    """a restatement that silently ran in float64 would make E = 0 and the GPU tolerance meaningless"""
    c = SINGLE_CASES[0]
    src = case_source(c)
    a = do.resample_f32(src, c[4], c[3], bool(c[5]), bool(c[6]), c[7])
    assert a.dtype == np.float32
    E = np.abs(a.astype(np.float64) - io.resample(src, c[4], c[3], bool(c[5]), bool(c[6]), c[7])).max()
    assert 2.0 ** -27 < E < 2.0 ** -18, E


# ------------------------------------------------------------------------------------------------------------------ 64-bit offsets
def test_input_kernels_assemble_64_bit_offsets_from_the_documented_words():
    """k_input_resample: params[1] << 32 | params[0] (one offset for both source kinds); k_color_jitter: var[n][1] << 32 | var[n][0];
    k_u8_to_f4: frames[1] << 32 | frames[0] (arena bytes) and frames[4] << 32 | frames[3] (float-buffer pixels).  Each word goes
    through uint32_t first (a negative low word must not sign-extend into the high one) and the shift happens in size_t."""
    with open(os.path.join(ROOT, "vae-cyclegan-implementation_amd", "csrc", "input.hip")) as f:
        text = f.read()
    pat = re.compile(r"\(\(size_t\)\(uint32_t\)(\w+)\[([^\]]+)\]\)\s*<<\s*32\s*\|\s*\(size_t\)\(uint32_t\)(\w+)\[([^\]]+)\]")
    found = [(m.group(1), m.group(2).replace(" ", ""), m.group(3), m.group(4).replace(" ", "")) for m in pat.finditer(text)]
    assert found == [("q", "1", "q", "0"), ("var", "n*4+1", "var", "n*4"), ("q", "1", "q", "0"), ("q", "4", "q", "3")], found
    assert len(re.findall(r"<<\s*32", text)) == 4                              # no other, differently written, assembly
    # the float-buffer offset is applied to a float4 pointer (pixels), the arena offset to a byte pointer
    assert "const float4* fs = p.fsrc + (fl ? soff : 0);" in text and "const unsigned char* src = p.arena + soff;" in text
    assert re.search(r"float4\* px = reinterpret_cast<float4\*>\(img\) \+ \(var \?", text)
    assert re.search(r"float4\* dst = fbuf \+ \(", text)
