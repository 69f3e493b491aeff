"""The PNG encoder's stream restated in numpy / Python from the comment of include/vicasplat_png.h alone: the yardstick of
tests/test_png_cpu.py and tests/test_png_gpu.py.  It also builds the cases and plants the defects.

encode(pixels, mode, defect=None) -> the file's bytes.  pixels: uint8 [H, W, C], C in (1, 3, 4).  mode: 0 .. 4 or ADAPTIVE.
"""
import functools
import os
import struct
import zlib

import numpy as np

ADAPTIVE = 5
SEGMENT_BYTES = 16384
SIGNATURE = bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
# "paeth_b_before_a" is planted too (paeth), but no decoder can see it: pa == pb with a != b means p == c, and c wins either way
# (test_png_cpu proves it over all byte triples).  The tie order that can be seen is the one between b and c.
DEFECTS = ("paeth_c_before_b", "average_rounds_up", "adler_without_modulus", "crc_without_type", "huffman_lsb_first", "extra_bits_msb_first",
           "run_piece_259", "no_end_of_block", "kraft_above_one", "hlit_off_by_one", "sync_nlen_not_complement")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_frames.npz")


class Refused(ValueError):
    pass


# ---- shape --------------------------------------------------------------------------------------------------------------------------------
def shape(h, w, c):
    """(rb, R, S): bytes of a filtered row, rows per segment, segments."""
    if c not in (1, 3, 4) or h < 1 or w < 1:
        raise Refused(f"{h} x {w} x {c}")
    rb = 1 + w * c
    if rb > 65535 or h > 65535:
        raise Refused(f"a row of {rb} bytes, {h} rows")
    rows = min(max(SEGMENT_BYTES // rb, 1), h)
    return rb, rows, -(-h // rows)


def bound(h, w, c):
    rb, _, segs = shape(h, w, c)
    return 51 + h * rb + 22 * segs


def quantise(x):
    """uint8(trunc(min(max(x, 0), 1) * 255)) in f32; a NaN gives 0."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(x), np.float32(0), np.minimum(np.maximum(x, np.float32(0)), np.float32(1)))
        return np.trunc(v.astype(np.float32) * np.float32(255)).astype(np.uint8)


# ---- filters ------------------------------------------------------------------------------------------------------------------------------
def paeth(a, b, c, defect=None):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    if defect == "paeth_b_before_a":
        return np.where((pb <= pa) & (pb <= pc), b, np.where(pa <= pc, a, c))
    if defect == "paeth_c_before_b":
        return np.where((pa <= pb) & (pa <= pc), a, np.where(pb < pc, b, c))
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(pixels, mode, defect=None):
    """(filtered stream uint8 [H, rb], the row types)."""
    h, w, c = pixels.shape
    x = pixels.reshape(h, w * c).astype(np.int32)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c] if w > 1 else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    cc = np.zeros_like(x)
    cc[1:, c:] = x[:-1, :-c] if w > 1 else 0
    avg = (a + b + (1 if defect == "average_rounds_up" else 0)) >> 1
    cand = np.stack([x, x - a, x - b, x - avg, x - paeth(a, b, cc, defect)]) & 255      # [5, H, W C]
    if mode == ADAPTIVE:
        cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                         # [5, H]
        types = cost.argmin(axis=0)                                                      # the first minimum: the lowest type on a tie
    else:
        types = np.full(h, mode)
    rows = cand[types, np.arange(h)]
    return np.concatenate([types[:, None], rows], axis=1).astype(np.uint8), [int(t) for t in types]


# ---- tokens -------------------------------------------------------------------------------------------------------------------------------
def tokens(seg, piece=258):
    """[(byte, None) for a literal, (None, length) for a match] of one segment's bytes."""
    seg = np.frombuffer(bytes(seg), np.uint8)
    cuts = np.flatnonzero(np.diff(seg)) + 1
    starts = np.concatenate([[0], cuts])
    ends = np.concatenate([cuts, [len(seg)]])
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        v = int(seg[s])
        out.append((v, None))
        rest = e - s - 1
        while rest >= piece:
            out.append((None, piece))
            rest -= piece
        if rest >= 3:
            out.append((None, rest))
        else:
            out.extend([(v, None)] * rest)
    return out


def length_symbol(n):
    """(symbol, extra value, extra bit count) of a match length."""
    k = max(i for i, base in enumerate(LENGTH_BASE) if base <= min(n, 258))
    return 257 + k, n - LENGTH_BASE[k] if k < 28 else 0, LENGTH_EXTRA[k]


# ---- codes --------------------------------------------------------------------------------------------------------------------------------
def huffman_depths(freq):
    """The leaf depths of the two-queue tree over the used symbols in (frequency, symbol) order: (order, depths in that order)."""
    order = sorted((s for s, f in enumerate(freq) if f > 0), key=lambda s: (freq[s], s))
    if len(order) < 2:
        return order, [1] * len(order)
    leaves = [(freq[s], ("leaf", i)) for i, s in enumerate(order)]
    merged, children = [], []
    li = mi = 0

    def pop():
        nonlocal li, mi
        if li < len(leaves) and (mi >= len(merged) or leaves[li][0] <= merged[mi][0]):
            li += 1
            return leaves[li - 1]
        mi += 1
        return merged[mi - 1]
    while (len(leaves) - li) + (len(merged) - mi) > 1:
        x, y = pop(), pop()
        children.append((x[1], y[1]))
        merged.append((x[0] + y[0], ("node", len(children) - 1)))
    depths = [0] * len(order)
    stack = [(("node", len(children) - 1), 0)]
    while stack:
        (kind, i), d = stack.pop()
        if kind == "leaf":
            depths[i] = d
        else:
            stack.extend((child, d + 1) for child in children[i])
    return order, depths


def code_lengths(freq, limit, defect=None):
    order, depths = huffman_depths(freq)
    lengths = [0] * len(freq)
    if len(order) < 2:
        for s in order:
            lengths[s] = 1
        return lengths
    n = [0] * (max(max(depths), limit) + 1)
    for d in depths:
        n[d] += 1
    n[limit] += sum(n[limit + 1:])
    del n[limit + 1:]
    kraft = sum(n[d] << (limit - d) for d in range(1, limit + 1))
    while kraft > (1 << limit) and defect != "kraft_above_one":
        n[limit] -= 1
        d = max(d for d in range(1, limit) if n[d] > 0)
        n[d] -= 1
        n[d + 1] += 2
        kraft -= 1
    at = 0
    for d in range(limit, 0, -1):
        for _ in range(n[d]):
            lengths[order[at]] = d
            at += 1
    return lengths


def canonical(lengths):
    """{symbol: (code, length)} per RFC 1951 3.2.2."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def clen_sequence(lengths):
    """[(symbol, extra value)] of the run-length coded code lengths."""
    seq, i = [], 0
    while i < len(lengths):
        v, j = lengths[i], i
        while j < len(lengths) and lengths[j] == v:
            j += 1
        r, i = j - i, j
        if v == 0:
            while r >= 138:
                seq.append((18, 138 - 11))
                r -= 138
            if r >= 11:
                seq.append((18, r - 11))
            elif r >= 3:
                seq.append((17, r - 3))
            else:
                seq.extend([(0, 0)] * r)
        else:
            seq.append((v, 0))
            r -= 1
            while r >= 6:
                seq.append((16, 3))
                r -= 6
            if r >= 3:
                seq.append((16, r - 3))
            else:
                seq.extend([(v, 0)] * r)
    return seq


class Bits:
    def __init__(self, defect=None):
        self.out, self.acc, self.n, self.defect = bytearray(), 0, 0, defect

    def field(self, value, count):          # least significant bit first
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def extra(self, value, count):
        if self.defect == "extra_bits_msb_first":
            value = int(format(value, f"0{count}b")[::-1], 2) if count else 0
        self.field(value, count)

    def code(self, pair):                   # a Huffman code: most significant bit first
        code, length = pair
        if self.defect != "huffman_lsb_first":
            code = int(format(code, f"0{length}b")[::-1], 2)
        self.field(code, length)

    def align(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc = self.n = 0


FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def plan_segment(seg, defect=None):
    """Everything the block decision needs: dict(tokens, freq, lengths, seq, clen, bits = {form: bit count}, form)."""
    toks = tokens(seg, 259 if defect == "run_piece_259" else 258)
    freq, matches, extra = [0] * 286, 0, 0
    for v, n in toks:
        if n is None:
            freq[v] += 1
        else:
            sym, _, ne = length_symbol(n)
            freq[sym] += 1
            matches += 1
            extra += ne
    freq[256] = 1
    lengths = code_lengths(freq, 15, defect)
    nlit = max(s for s in range(286) if lengths[s]) + 1
    dist = 1 if matches else 0
    seq = clen_sequence(lengths[:nlit] + [dist])
    cfreq = [0] * 19
    for s, _ in seq:
        cfreq[s] += 1
    clen = code_lengths(cfreq, 7, defect)
    nclen = max([4] + [k + 1 for k in range(19) if clen[CLEN_ORDER[k]]])
    dynamic = 3 + 14 + 3 * nclen + sum(clen[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in seq) + \
        sum(f * l for f, l in zip(freq, lengths)) + extra + matches
    fixed = 3 + sum(f * l for f, l in zip(freq, FIXED_LENGTHS)) + extra + 5 * matches
    stored = 40 + 8 * len(seg)
    form = "stored" if stored <= fixed and stored <= dynamic else ("fixed" if fixed <= dynamic else "dynamic")
    return dict(tokens=toks, freq=freq, lengths=lengths, nlit=nlit, dist=dist, seq=seq, clen=clen, nclen=nclen,
                bits=dict(stored=stored, fixed=fixed, dynamic=dynamic), form=form)


def encode_segment(seg, last, defect=None):
    """The deflate bytes of one segment (they start and end on a byte)."""
    seg = bytes(seg)
    p = plan_segment(seg, defect)
    w = Bits(defect)
    w.field((1 if last else 0) | ({"stored": 0, "fixed": 1, "dynamic": 2}[p["form"]] << 1), 3)
    if p["form"] == "stored":
        w.align()
        w.out += struct.pack("<HH", len(seg), len(seg) ^ 0xFFFF) + seg
    else:
        if p["form"] == "fixed":
            lit, dist = canonical(FIXED_LENGTHS), (0, 5)
        else:
            lit, dist, cc = canonical(p["lengths"]), (0, 1), canonical(p["clen"])
            w.field(p["nlit"] - 257 + (1 if defect == "hlit_off_by_one" else 0), 5)
            w.field(0, 5)
            w.field(p["nclen"] - 4, 4)
            for k in range(p["nclen"]):
                w.field(p["clen"][CLEN_ORDER[k]], 3)
            for s, e in p["seq"]:
                w.code(cc[s])
                if s >= 16:
                    w.field(e, {16: 2, 17: 3, 18: 7}[s])
        for v, n in p["tokens"]:
            if n is None:
                w.code(lit[v])
            else:
                sym, e, ne = length_symbol(n)
                w.code(lit[sym])
                w.extra(e, ne)
                w.code(dist)
        if defect != "no_end_of_block":
            w.code(lit[256])
    if last:
        w.align()
    else:
        w.field(0, 3)
        w.align()
        w.out += b"\x00\x00\x00\x00" if defect == "sync_nlen_not_complement" else b"\x00\x00\xff\xff"
    return bytes(w.out)


def adler32(data, defect=None):
    sums = 1 + np.cumsum(np.frombuffer(data, np.uint8).astype(np.uint64))          # a after every byte; b is their sum
    a, b = int(sums[-1]), int(sums.sum())
    if defect == "adler_without_modulus":
        return ((b & 0xFFFF) << 16) | (a & 0xFFFF)
    return ((b % 65521) << 16) | (a % 65521)


def chunk(kind, data, defect=None):
    crc = zlib.crc32(data) if defect == "crc_without_type" else zlib.crc32(kind + data)
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc)


def segments(stream, h, w, c):
    """The filtered stream [H, rb] cut into the segments' byte strings."""
    _, rows, segs = shape(h, w, c)
    return [stream[k * rows:(k + 1) * rows].tobytes() for k in range(segs)]


def encode(pixels, mode=ADAPTIVE, defect=None):
    pixels = np.ascontiguousarray(pixels, np.uint8)
    h, w, c = pixels.shape
    shape(h, w, c)
    stream, _ = filter_rows(pixels, mode, defect)
    segs = segments(stream, h, w, c)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, {1: 0, 3: 2, 4: 6}[c], 0, 0, 0), defect)
    for k, seg in enumerate(segs):
        data = encode_segment(seg, k == len(segs) - 1, defect)
        if k == 0:
            data = b"\x78\x01" + data
        if k == len(segs) - 1:
            data += struct.pack(">I", adler32(stream.tobytes(), defect))
        out += chunk(b"IDAT", data, defect)
    return out + chunk(b"IEND", b"", defect)


def chunks(data):
    """[(type, data, stored crc)] of a file."""
    assert data[:8] == SIGNATURE
    out, at = [], 8
    while at < len(data):
        n, = struct.unpack_from(">I", data, at)
        out.append((data[at + 4:at + 8], data[at + 8:at + 8 + n], struct.unpack_from(">I", data, at + 8 + n)[0]))
        at += 12 + n
    assert at == len(data)
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng(seed)


def _smooth(h, w, c, seed):
    """A smooth picture with a little noise: the dynamic form wins on it."""
    r = _rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [127 + 90 * np.sin(x / (7.0 + k) + k) * np.cos(y / (11.0 - k)) + r.integers(-3, 4, (h, w)) for k in range(c)]
    return np.clip(np.stack(planes, -1), 0, 255).astype(np.uint8)


def _spread(counts):
    """A byte string with counts[v] bytes of value v and no two equal neighbours (the largest count is at most half of all, rounded up)."""
    values = [v for v, n in sorted(counts.items(), key=lambda kv: -kv[1]) for _ in range(n)]
    out = [0] * len(values)
    slots = list(range(0, len(values), 2)) + list(range(1, len(values), 2))
    for slot, v in zip(slots, values):
        out[slot] = v
    return out


def _grey_row(values):
    return np.asarray(values, np.uint8).reshape(1, -1, 1)


RUNS = (2, 3, 4, 258, 259, 260, 261, 262, 517)


def _runs_row():
    values = []
    for k, n in enumerate(RUNS):
        values += [100 + k] * n + [200 + k, 50 + k]          # the run, then two bytes that differ from it and from each other
    return _grey_row([9] + values)                            # (the filter byte 0 stands alone in front)


def fibonacci_counts():
    fib = [1, 1]
    while fib[-1] < 4181:
        fib.append(fib[-1] + fib[-2])
    return fib


def _fibonacci_row():
    """Symbol counts 1, 1, 2, 3, ..., 4181: the filter byte 0 and the end-of-block symbol are the two 1s, pixel values 1 .. 17 the others."""
    return _grey_row(_spread({k + 1: n for k, n in enumerate(fibonacci_counts()[2:])}))


def _all_symbols_row():
    """All 256 literals and a match of every length symbol, in a segment the dynamic form wins."""
    values = list(range(1, 256))                              # 0 is the filter byte
    for k, base in enumerate(LENGTH_BASE):
        values += [(2 * k + 1) % 256] * (base + 1) + [(2 * k + 2) % 256 or 7]
    values += _spread({10: 1500, 20: 1500, 30: 1000})          # a skew that makes the dynamic form the smallest
    return _grey_row(values)


# Literal/length code lengths and the number of PIXEL VALUES that get each.  With the filter byte and the end-of-block symbol, which occur once
# and so sit at length 13, the lengths satisfy sum n 2^-L = 1, and a value of length L occurs 2^(13 - L) times: the Huffman lengths are
# exactly these.  No two neighbouring symbols share a length, so the code-length alphabet sees the frequencies 18: 1, 0: 1, 2: 2, 3: 3, 7: 5,
# 8: 8, 12: 13, 10: 21, 13: 34, 11: 55 -- Fibonacci numbers, whose tree is 9 deep.
CLEN_LIMIT_PLAN = {2: 2, 3: 3, 7: 5, 8: 8, 10: 21, 11: 55, 12: 13, 13: 32}


def _clen_limit_row():
    lengths = _spread(CLEN_LIMIT_PLAN)
    return _grey_row(_spread({value + 1: 1 << (13 - length) for value, length in enumerate(lengths)}))


def _each_filter_rows(c=3, w=24):
    """Rows built so that the adaptive rule picks every type: small raw values that a left neighbour only doubles, a ramp under a row of
    zeros, a copy of the row above, the exact average, the exact Paeth predictor (one pixel aside, so that it is no copy)."""
    r = _rng(7)
    n = w * c
    rows = [3 * ((np.arange(n) // c) % 2)]                                       # none: `up` ties in row 0, every other type costs more
    rows.append(np.zeros(n, np.int64))
    rows.append((40 + 5 * (np.arange(n) // c) + 60 * (np.arange(n) % c)) % 256)  # sub: under zeros Paeth predicts the left byte too, a tie
    rows.append(r.integers(0, 256, n))
    rows.append(rows[-1].copy())                                                # up
    above = rows[-1]
    avg = np.zeros(n, np.int64)
    for j in range(n):
        avg[j] = ((avg[j - c] if j >= c else 0) + above[j]) >> 1
    rows.append(avg)                                                            # average
    rows.append(r.integers(0, 256, n))
    above = rows[-1]
    pa = np.zeros(n, np.int64)
    for j in range(n):
        a, b, cc = (pa[j - c] if j >= c else 0), above[j], (above[j - c] if j >= c else 0)
        p = a + b - cc
        da, db, dc = abs(p - a), abs(p - b), abs(p - cc)
        pa[j] = ((a if da <= db and da <= dc else (b if db <= dc else cc)) + (9 if c <= j < 2 * c else 0)) % 256
    rows.append(pa)                                                             # paeth
    return np.stack(rows).astype(np.uint8).reshape(len(rows), w, c)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (pixels uint8 [H, W, C], filter mode)}."""
    r = _rng(1)
    rows = shape(64, 256, 3)[1]
    out = {}
    for c in (1, 3, 4):
        out[f"1x1_c{c}"] = (r.integers(0, 256, (1, 1, c), dtype=np.uint8), ADAPTIVE)
    out["1x7"] = (r.integers(0, 256, (1, 7, 3), dtype=np.uint8), ADAPTIVE)
    out["7x1"] = (r.integers(0, 256, (7, 1, 3), dtype=np.uint8), ADAPTIVE)
    for name, h in (("R-1", rows - 1), ("R", rows), ("R+1", rows + 1), ("2R+1", 2 * rows + 1)):
        out[f"256_rgb_{name}"] = (_smooth(h, 256, 3, h), ADAPTIVE)
    long_row = np.zeros((2, 65534, 1), np.uint8)
    long_row[0, :, 0] = (np.arange(65534) // 37) % 251
    long_row[1, :, 0] = (np.arange(65534) * 7 // 5) % 256
    out["long_row"] = (long_row, ADAPTIVE)
    out["runs"] = (_runs_row(), 0)
    out["constant_rgb"] = (np.full((256, 256, 3), 93, np.uint8), ADAPTIVE)
    out["constant_grey_zero"] = (np.zeros((1, 60 * 258, 1), np.uint8), 0)         # matches only: one literal, then 60 x 258
    out["two_symbols"] = (np.zeros((1, 1, 1), np.uint8), 0)
    out["noise"] = (r.integers(0, 256, (64, 64, 3), dtype=np.uint8), ADAPTIVE)
    out["fibonacci"] = (_fibonacci_row(), 0)
    out["clen_limit"] = (_clen_limit_row(), 0)
    out["all_symbols"] = (_all_symbols_row(), 0)
    out["no_match"] = (_grey_row(_spread({v: 8 for v in range(1, 40)})), 0)
    for mode in range(5):
        out[f"fixed_filter_{mode}"] = (_smooth(9, 11, 4 if mode % 2 else 3, 20 + mode), mode)
    out["each_filter"] = (_each_filter_rows(), ADAPTIVE)
    out["rgba"] = (_smooth(33, 40, 4, 3), ADAPTIVE)
    if os.path.exists(GOLDEN):
        z = np.load(GOLDEN)
        out["golden_frame"] = (z["frame"], ADAPTIVE)
        out["golden_small_rgb"] = (z["small_rgb"], ADAPTIVE)
        out["golden_small_grey"] = (z["small_grey"], ADAPTIVE)
    return out


@functools.lru_cache(maxsize=None)
def reference_file(name):
    pixels, mode = cases()[name]
    return encode(pixels, mode)


# the cases of one shape that the GPU tests batch: two mixed batches of 5
def batches():
    r = _rng(11)
    a = [_smooth(23, 40, 3, 100), np.full((23, 40, 3), 200, np.uint8), r.integers(0, 256, (23, 40, 3), dtype=np.uint8),
         _smooth(23, 40, 3, 101), np.zeros((23, 40, 3), np.uint8)]
    b = [_smooth(45, 250, 1, 102), r.integers(0, 256, (45, 250, 1), dtype=np.uint8), np.full((45, 250, 1), 1, np.uint8),
         _smooth(45, 250, 1, 103), (np.arange(45 * 250).reshape(45, 250, 1) % 256).astype(np.uint8)]
    return {"23x40_rgb": np.stack(a), "45x250_grey": np.stack(b)}


def float_probes():
    """The f32 values at which the quantisation can go wrong."""
    one = np.float32(1)
    eps = np.float32(2.0 ** -23)
    ks = np.arange(0, 256, dtype=np.float32) / np.float32(255)
    vals = [np.float32(0), one, -np.float32(0), np.float32(np.inf), -np.float32(np.inf), np.float32(np.nan), np.float32(0.5), np.float32(-1e-30),
            np.float32(1e-30), np.float32(1.0000001), np.float32(0.99999994)]
    return np.concatenate([np.asarray(vals, np.float32), ks, ks * (one + eps), ks * (one - eps), np.nextafter(ks, np.float32(-1)),
                           np.nextafter(ks, np.float32(2))]).astype(np.float32)
