"""The yardstick of the JPEG decoder: a plain numpy / Python restatement of the whole decode -- marker walk, Huffman decode bit by bit,
libjpeg's islow inverse DCT, fancy chroma upsampling and YCbCr -> RGB --, written from the algorithm as include/vicasplat_jpeg.h states it,
not from the package's code.  tests/test_jpeg_cpu.py pins it to the installed PIL on every case, 0 differing bytes.

Also here: the case list (the smallest images at which each path can go wrong; "w x h"), the deterministic images they encode, the
descriptors and tables in the header's formats (compared with the package's host parser), the damaged variants of a stream, and the planted
defects (`mutant=`), each of which must change at least one byte of at least one case.
"""
from __future__ import annotations

import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")

MUTANTS = ("plus7_for_plus8", "fancy_at_width_2", "padded_width", "padded_bottom_row", "descale_no_rounding", "idct_constant",
           "colour_no_half", "dc_not_reset", "stuffing_kept", "extend_off_by_one")

S444, S422, S420 = 0, 1, 2      # PIL's `subsampling`

# name -> (w, h, content, mode, save arguments)
CASES = {
    "1x1": (1, 1, "noise", "RGB", dict(quality=90, subsampling=S444)),
    "8x8": (8, 8, "noise", "RGB", dict(quality=90, subsampling=S444)),
    "9x9_444": (9, 9, "ramp", "RGB", dict(quality=50, subsampling=S444)),
    "9x9_420": (9, 9, "noise", "RGB", dict(quality=90, subsampling=S420)),
    "16x16_420": (16, 16, "noise", "RGB", dict(quality=90, subsampling=S420)),
    "16x16_checker": (16, 16, "checker", "RGB", dict(quality=90, subsampling=S420)),
    "17x17_420": (17, 17, "noise", "RGB", dict(quality=90, subsampling=S420)),
    "17x17_checker_422": (17, 17, "checker", "RGB", dict(quality=50, subsampling=S422)),
    "3x5_420": (3, 5, "noise", "RGB", dict(quality=90, subsampling=S420)),
    "3x5_422": (3, 5, "noise", "RGB", dict(quality=90, subsampling=S422)),
    "4x2_420": (4, 2, "noise", "RGB", dict(quality=90, subsampling=S420)),
    "4x2_422": (4, 2, "noise", "RGB", dict(quality=90, subsampling=S422)),
    "5x5_420": (5, 5, "noise", "RGB", dict(quality=90, subsampling=S420)),
    "5x5_422": (5, 5, "noise", "RGB", dict(quality=90, subsampling=S422)),
    "6x3_422": (6, 3, "noise", "RGB", dict(quality=90, subsampling=S422)),
    "10x6_420": (10, 6, "noise", "RGB", dict(quality=90, subsampling=S420)),      # an even height whose last chroma row is not a block's last
    "13x11_gray": (13, 11, "noise", "L", dict(quality=90)),
    "8x8_zero": (8, 8, "c0", "RGB", dict(quality=90, subsampling=S420)),
    "9x9_128": (9, 9, "c128", "RGB", dict(quality=50, subsampling=S422)),
    "8x8_255": (8, 8, "c255", "RGB", dict(quality=100, subsampling=S444)),
    "45x80_444": (45, 80, "noise", "RGB", dict(quality=90, subsampling=S444)),
    "45x80_422": (45, 80, "ramp", "RGB", dict(quality=90, subsampling=S422)),
    "45x80_420": (45, 80, "field", "RGB", dict(quality=90, subsampling=S420)),
    "45x80_q1": (45, 80, "noise", "RGB", dict(quality=1, subsampling=S420)),
    "45x80_q100": (45, 80, "noise", "RGB", dict(quality=100, subsampling=S422)),
    "80x45_444": (80, 45, "ramp", "RGB", dict(quality=50, subsampling=S444)),
    "80x45_422": (80, 45, "noise", "RGB", dict(quality=90, subsampling=S422)),
    "80x45_420": (80, 45, "noise", "RGB", dict(quality=90, subsampling=S420)),
    "80x45_rows": (80, 45, "field", "RGB", dict(quality=90, subsampling=S420, restart_marker_rows=1)),
    "80x45_optimize": (80, 45, "noise", "RGB", dict(quality=100, subsampling=S420, optimize=True)),
    "96x48_restart": (96, 48, "noise", "RGB", dict(quality=50, subsampling=S444, restart_marker_blocks=1)),
}
# batches of five frames of one size with different sampling, tables and restart settings
BATCHES = {
    "45x80": ("45x80_444", "45x80_422", "45x80_420", "45x80_q1", "45x80_q100"),
    "80x45": ("80x45_444", "80x45_422", "80x45_rows", "80x45_optimize", "80x45_420"),
}
# the damaged batch of the GPU test: (case, kind, argument) per frame; see `damage`
DAMAGED_BATCH = (("80x45_444", None, 0), ("80x45_422", None, 0), ("80x45_420", "truncate", 0.5), ("80x45_optimize", None, 0), ("80x45_rows", "flip", 2))


def make_image(content: str, w: int, h: int, mode: str, seed: int = 0) -> np.ndarray:
    """uint8 [h, w, 3] (or [h, w] for mode "L"), deterministic."""
    g = np.random.default_rng([seed, w, h, len(content)])
    ch = 1 if mode == "L" else 3
    y, x = np.mgrid[0:h, 0:w]
    if content == "noise":
        a = g.integers(0, 256, (h, w, ch))
    elif content == "ramp":
        a = np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)][:ch], -1)
    elif content == "field":      # a smooth field plus mild noise
        a = np.stack([128 + 100 * np.sin(x / 9.0 + c) * np.cos(y / 7.0 - c) for c in range(ch)], -1) + g.normal(0, 6, (h, w, ch))
    elif content == "checker":
        a = np.repeat((((x + y) & 1) * 255)[..., None], ch, -1)
    else:
        a = np.full((h, w, ch), int(content[1:]))
    a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return a[..., 0] if mode == "L" else a


def encode(name: str) -> bytes:
    from PIL import Image
    w, h, content, mode, kw = CASES[name]
    buf = io.BytesIO()
    Image.fromarray(make_image(content, w, h, mode), mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_decode(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


_fixture = None


def fixture() -> dict:
    """{case: (stream bytes, PIL's pixels uint8 [h, w, 3])} of tests/golden/jpeg_cases.npz."""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        _fixture = {name: (z[name + ".jpg"].tobytes(), z[name + ".rgb"]) for name in CASES}
    return _fixture


# ---- the marker walk ------------------------------------------------------------------------------------------------------------------
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


def parse(data: bytes) -> dict:
    """The frame's header and restart segments.  Only what the cases need: a stream outside the scope raises ValueError."""
    assert data[:2] == b"\xff\xd8"
    pos, quant, huff, ri, frame = 2, {}, {}, 0, None
    while True:
        assert data[pos] == 0xFF
        m, size = data[pos + 1], data[pos + 2] * 256 + data[pos + 3]
        body = data[pos + 4: pos + 2 + size]
        pos += 2 + size
        if m == 0xDB:
            for at in range(0, len(body), 65):
                assert body[at] < 16
                quant[body[at]] = body[at + 1: at + 65]
        elif m == 0xC4:
            at = 0
            while at < len(body):
                n = sum(body[at + 1: at + 17])
                huff[body[at]] = body[at + 1: at + 17 + n]
                at += 17 + n
        elif m in (0xC0, 0xC1):
            assert body[0] == 8
            frame = (body[1] * 256 + body[2], body[3] * 256 + body[4], [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i])
                                                                        for i in range(body[5])])
        elif m == 0xDD:
            ri = body[0] * 256 + body[1]
        elif m == 0xDA:
            break
        elif not 0xE0 <= m <= 0xEF and m != 0xFE:
            raise ValueError(f"marker FF{m:02X}")
    h, w, comps = frame
    ncomp = len(comps)
    assert body[0] == ncomp and [body[1 + 2 * i] for i in range(ncomp)] == [c[0] for c in comps]
    hs, vs = (1, 1) if ncomp == 1 else comps[0][1:3]
    mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
    # the entropy-coded data: up to the first marker that is no RSTn
    begins, ends, p = [pos], [], pos
    while True:
        p = data.find(b"\xff", p)
        if p < 0 or p + 1 >= len(data):
            raise ValueError("missing EOI")
        nxt = data[p + 1]
        if nxt == 0 or nxt == 0xFF:
            p += 1
            continue
        e = p
        while e > begins[-1] and data[e - 1] == 0xFF:      # fill bytes
            e -= 1
        ends.append(e)
        if 0xD0 <= nxt <= 0xD7:
            begins.append(p + 2)
            p += 2
            continue
        if nxt != 0xD9:
            raise ValueError(f"marker FF{nxt:02X} in the scan")
        break
    total = mx * my
    per = ri or total
    if len(begins) != -(-total // per):
        raise ValueError("restart markers do not match the interval")
    segs = [(begins[i], ends[i], i * per, min(per, total - i * per)) for i in range(len(begins))]
    return dict(h=h, w=w, ncomp=ncomp, hs=hs, vs=vs, mx=mx, my=my, ri=ri, segs=segs,
                quant=[bytes(quant[c[3]]) for c in comps],
                dc=[bytes(huff[body[2 + 2 * i] >> 4]) for i in range(ncomp)],
                ac=[bytes(huff[0x10 | (body[2 + 2 * i] & 15)]) for i in range(ncomp)])


def codes_of(payload: bytes) -> dict:
    """{(length, code): symbol} of a DHT payload (16 counts, then the symbols): the canonical code."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(payload[length - 1]):
            out[length, code] = payload[16 + k]
            code += 1
            k += 1
        code <<= 1
    return out


# ---- the entropy decode ---------------------------------------------------------------------------------------------------------------
INDEX, CODE, SHORT, LEFTOVER, MARKER = 1, 2, 4, 8, 16


class _Bits:
    def __init__(self, raw: bytes, mutant):
        self.status = 0
        out, i = bytearray(), 0
        while i < len(raw):
            b = raw[i]
            i += 1
            if b == 0xFF:
                if i < len(raw) and raw[i] == 0:
                    if mutant != "stuffing_kept":
                        i += 1
                else:
                    self.status |= MARKER
                    break
            out.append(b)
        self.bits = np.unpackbits(np.frombuffer(bytes(out), np.uint8)).tolist()
        self.at = 0

    def take(self, n: int) -> int:
        v = 0
        for _ in range(n):
            v = (v << 1) | (self.bits[self.at] if self.at < len(self.bits) else 0)
            self.at += 1
        return v

    def symbol(self, table: dict) -> int:
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in table:
                return table[length, code]
        self.status |= CODE
        return -1


def _extend(v: int, s: int, mutant) -> int:
    if s == 0:
        return 0
    if mutant == "extend_off_by_one":
        return v if v > 1 << (s - 1) else v - (1 << s) + 1
    return v if v >= 1 << (s - 1) else v - (1 << s) + 1


def _block(br: _Bits, dc: dict, ac: dict, pred: int, mutant):
    """(64 coefficients in natural order or None when the block is damaged, the new predictor)."""
    coef = [0] * 64
    s = br.symbol(dc)
    if s < 0:
        return None, pred
    pred = (pred + _extend(br.take(s & 15), s & 15, mutant) + 32768) % 65536 - 32768
    coef[0] = pred
    k = 1
    while k < 64:
        rs = br.symbol(ac)
        if rs < 0:
            return None, pred
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r != 15:
                break
            k += 16
            continue
        k += r
        if k > 63:
            br.status |= INDEX
            return None, pred
        coef[ZIGZAG[k]] = _extend(br.take(s), s, mutant)
        k += 1
    if k > 64:
        br.status |= INDEX
        return None, pred
    return coef, pred


def decode_coefficients(data: bytes, p: dict | None = None, mutant: str | None = None):
    """(per component int32 [blocks_y, blocks_x, 64] in natural order on the padded planes, status): 0 = clean, else the OR of the
    segments' bits.  A segment stops at its first damaged block; what it leaves out is zero."""
    p = p or parse(data)
    ncomp, hs, vs, mx, my = p["ncomp"], p["hs"], p["vs"], p["mx"], p["my"]
    fac = [(hs, vs)] + [(1, 1)] * (ncomp - 1)
    planes = [np.zeros((my * v, mx * hh, 64), np.int32) for hh, v in fac]
    dc, ac = [codes_of(t) for t in p["dc"]], [codes_of(t) for t in p["ac"]]
    status = 0
    pred = [0] * ncomp
    for begin, end, first, count in p["segs"]:
        br = _Bits(data[begin:end], mutant)
        if mutant != "dc_not_reset":
            pred = [0] * ncomp
        ok = True
        for m in range(first, first + count):
            for c in range(ncomp):
                for v in range(fac[c][1]):
                    for u in range(fac[c][0]):
                        if ok:
                            coef, pred[c] = _block(br, dc[c], ac[c], pred[c], mutant)
                            ok = coef is not None
                            if ok:
                                planes[c][(m // mx) * fac[c][1] + v, (m % mx) * fac[c][0] + u] = coef
        if ok:
            left = len(br.bits) - br.at
            if left < 0:
                br.status |= SHORT
            elif left >= 8:
                br.status |= LEFTOVER
        status |= br.status
    return planes, status


# ---- reconstruction -------------------------------------------------------------------------------------------------------------------
def _idct_pass(c, n: int, mutant):
    """One 8-point pass along the last axis of c [..., 8] (int64)."""
    k6270 = 6271 if mutant == "idct_constant" else 6270
    c0, c1, c2, c3, c4, c5, c6, c7 = (c[..., i] for i in range(8))
    z1 = (c2 + c6) * 4433
    tmp2, tmp3 = z1 - c6 * 15137, z1 + c2 * k6270
    tmp0, tmp1 = (c0 + c4) << 13, (c0 - c4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = c7, c5, c3, c1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)
    return (out + (0 if mutant == "descale_no_rounding" else 1 << (n - 1))) >> n


def idct_plane(coef: np.ndarray, quant_zigzag: bytes, mutant: str | None = None) -> np.ndarray:
    """coef [by, bx, 64] natural order -> the padded sample plane uint8 [8 by, 8 bx]."""
    q = np.zeros(64, np.int64)
    q[ZIGZAG] = np.frombuffer(quant_zigzag, np.uint8)
    by, bx, _ = coef.shape
    blocks = (coef.astype(np.int64) * q).reshape(by, bx, 8, 8)                              # [.., row, column]
    ws = np.swapaxes(_idct_pass(np.swapaxes(blocks, -1, -2), 11, mutant), -1, -2)         # columns first
    px = np.clip(_idct_pass(ws, 18, mutant) + 128, 0, 255).astype(np.uint8)
    return px.transpose(0, 2, 1, 3).reshape(8 * by, 8 * bx)


def _h2v1(rows: np.ndarray) -> np.ndarray:
    """Fancy 2 x 1 upsampling of rows [H, W'] (W' > 2) -> [H, 2 W']."""
    a = rows.astype(np.int64)
    n = a.shape[1]
    out = np.zeros((a.shape[0], 2 * n), np.int64)
    out[:, 0] = a[:, 0]
    out[:, 2::2] = (3 * a[:, 1:] + a[:, :-1] + 1) >> 2
    out[:, 1:-1:2] = (3 * a[:, :-1] + a[:, 1:] + 2) >> 2
    out[:, 2 * n - 1] = a[:, n - 1]
    return out


def _h2v2(plane: np.ndarray, mutant, context_below=None) -> np.ndarray:
    """Fancy 2 x 2 upsampling of plane [H', W'] (W' > 2) -> [2 H', 2 W'].  context_below: the row taken for row H' (the planted defect)."""
    a = plane.astype(np.int64)
    hc, n = a.shape
    up = np.concatenate([a[:1], a[:-1]])
    down = np.concatenate([a[1:], a[-1:] if context_below is None else context_below[None].astype(np.int64)])
    s = np.empty((2 * hc, n), np.int64)
    s[0::2], s[1::2] = 3 * a + up, 3 * a + down
    eight = 7 if mutant == "plus7_for_plus8" else 8
    out = np.zeros((2 * hc, 2 * n), np.int64)
    out[:, 0] = (4 * s[:, 0] + eight) >> 4
    out[:, 2::2] = (3 * s[:, 1:] + s[:, :-1] + eight) >> 4
    out[:, 1:-1:2] = (3 * s[:, :-1] + s[:, 1:] + 7) >> 4
    out[:, 2 * n - 1] = (4 * s[:, n - 1] + 7) >> 4
    return out


def upsample(plane: np.ndarray, hs: int, vs: int, h: int, w: int, mutant: str | None = None) -> np.ndarray:
    """A padded chroma plane -> [h, w] at the luma's resolution."""
    if hs == 1:
        return plane[:h, :w].astype(np.int64)
    wc, hc = -(-w // 2), (-(-h // 2) if vs == 2 else h)
    if mutant == "padded_width":
        wc = plane.shape[1]
    true = plane[:hc, :wc]
    if wc <= 2 and mutant != "fancy_at_width_2":
        out = np.repeat(np.repeat(true, 2, axis=1), vs, axis=0)
    elif vs == 1:
        out = _h2v1(true)
    else:
        below = plane[hc, :wc] if (mutant == "padded_bottom_row" and hc < plane.shape[0]) else None
        out = _h2v2(true, mutant, below)
    return out[:h, :w].astype(np.int64)


def reconstruct(p: dict, planes, mutant: str | None = None) -> np.ndarray:
    """Coefficients -> uint8 [h, w, 3]."""
    h, w = p["h"], p["w"]
    samples = [idct_plane(planes[c], p["quant"][c], mutant) for c in range(p["ncomp"])]
    y = samples[0][:h, :w].astype(np.int64)
    if p["ncomp"] == 1:
        return np.repeat(y[..., None], 3, -1).astype(np.uint8)
    cb = upsample(samples[1], p["hs"], p["vs"], h, w, mutant) - 128
    cr = upsample(samples[2], p["hs"], p["vs"], h, w, mutant) - 128
    half = 0 if mutant == "colour_no_half" else 32768
    r = y + ((91881 * cr + half) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + half) >> 16)
    b = y + ((116130 * cb + half) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data: bytes, mutant: str | None = None):
    """(uint8 [h, w, 3], status) of one stream."""
    p = parse(data)
    planes, status = decode_coefficients(data, p, mutant)
    return reconstruct(p, planes, mutant), status


# ---- the header's formats: descriptors and tables of a batch ------------------------------------------------------------------------------
FRAME_WORDS, HUFF_BYTES, LOOK_BITS = 24, 1424, 9


def huffman_table(payload: bytes) -> np.ndarray:
    """The decode table of include/vicasplat_jpeg.h, from the codes themselves."""
    look = np.zeros(1 << LOOK_BITS, np.uint16)
    maxcode, valoff, vals = np.full(18, -1, np.int32), np.zeros(18, np.int32), np.zeros(256, np.uint8)
    order = sorted(codes_of(payload).items())      # by (length, code): the code order
    for k, ((length, code), sym) in enumerate(order):
        vals[k] = sym
        maxcode[length] = max(maxcode[length], code)
        if all(l2 != length for (l2, _), _ in order[:k]):
            valoff[length] = k - code
        if length <= LOOK_BITS:
            for tail in range(1 << (LOOK_BITS - length)):
                look[(code << (LOOK_BITS - length)) | tail] = (length << 8) | sym
    return np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), vals])


def descriptors(datas) -> dict:
    """frames [N, 24], segs [S, 4] (byte offsets into the concatenation of the streams), quant [Q, 64] uint16 natural order and huff
    [H, 1424] of a batch; tables are numbered in the order of their first use: per frame, per component, quantisation, DC, AC."""
    frames, segs, quant, huff, off, block0 = [], [], {}, {}, 0, 0
    for d in datas:
        p = parse(d)
        row = [0] * FRAME_WORDS
        row[:8] = [p["ncomp"], p["hs"], p["vs"], p["mx"], p["my"], len(segs), len(p["segs"]), block0]
        for c in range(p["ncomp"]):
            row[8 + c] = quant.setdefault(p["quant"][c], len(quant))
            row[11 + c] = huff.setdefault(p["dc"][c], len(huff))
            row[14 + c] = huff.setdefault(p["ac"][c], len(huff))
        frames.append(row)
        segs += [(b + off, e + off, first, count) for b, e, first, count in p["segs"]]
        off += len(d)
        block0 += p["mx"] * p["my"] * (p["hs"] * p["vs"] + (2 if p["ncomp"] == 3 else 0))
    qt = np.zeros((len(quant), 64), np.uint16)
    for payload, i in quant.items():
        qt[i, ZIGZAG] = np.frombuffer(payload, np.uint8)
    return dict(frames=np.array(frames, np.int32), segs=np.array(segs, np.int32), quant=qt,
                huff=np.stack([huffman_table(t) for t in huff]), blocks=block0)


# ---- damaged streams ------------------------------------------------------------------------------------------------------------------
def scan_range(data: bytes) -> tuple[int, int]:
    p = parse(data)
    return p["segs"][0][0], p["segs"][-1][1]


def damage(data: bytes, kind: str | None, arg) -> bytes:
    """A damaged copy: "truncate" cuts the scan at the fraction `arg` of its length (the EOI marker is kept behind the cut), "flip" inverts
    one bit of the scan chosen by the seed `arg`.  None: the stream itself."""
    if kind is None:
        return data
    a, b = scan_range(data)
    if kind == "truncate":
        cut = a + int((b - a) * arg) if isinstance(arg, float) else a + arg
        return data[:cut] + b"\xff\xd9"
    g = np.random.default_rng([arg, len(data)])
    at, bit = int(g.integers(a, b)), int(g.integers(0, 8))
    return data[:at] + bytes([data[at] ^ (1 << bit)]) + data[at + 1:]
