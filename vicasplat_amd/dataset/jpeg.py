"""JPEG decoding on the HIP path: the reference's `convert_images` (src/dataset/dataset_re10k.py: PIL's Image.open per frame, then ToTensor)
with the pixels produced on the device by vsj_decode (csrc/jpeg.hip, include/vicasplat_jpeg.h), byte for byte what PIL's libjpeg-turbo
gives.  The host walks each frame's markers -- a few hundred header bytes --, finds the restart markers of all frames with one vectorised
search, and hands the device ONE packed buffer: descriptors, tables and the compressed bytes.  There is no fallback to PIL.

Decoded: 8-bit baseline Huffman JPEG (SOF0 / SOF1), one interleaved scan, grayscale or YCbCr at 4:4:4, 4:2:2 or 4:2:0, any restart interval.
Everything else is refused by `pack_jpeg_batch` with a JpegError (an OSError, as PIL's own refusals are: a reader's
`except OSError: skip the example` behaves as the reference's does) that names the frame and the reason.  A grayscale frame comes back
with R = G = B = Y, which is what `Image.open(...).convert("RGB")` gives.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch
from torch import Tensor

from .. import _lib as L
from .shims.crop_shim import rescale

FRAME_WORDS, SEG_WORDS, HUFF_BYTES, LOOK_BITS = L.VSJ_FRAME_WORDS, L.VSJ_SEG_WORDS, L.VSJ_HUFF_BYTES, L.VSJ_LOOK_BITS
STATUS_BITS = {"INDEX": L.VSJ_STATUS_INDEX, "CODE": L.VSJ_STATUS_CODE, "SHORT": L.VSJ_STATUS_SHORT, "LEFTOVER": L.VSJ_STATUS_LEFTOVER,
               "MARKER": L.VSJ_STATUS_MARKER, "DESC": L.VSJ_STATUS_DESC}

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class JpegError(OSError):
    """A stream this decoder does not take, or one whose entropy-coded data is damaged.  `reason` is the bare reason, `frames` the indices
    of the frames concerned within the call."""

    def __init__(self, reason: str, frames=()):
        self.reason, self.frames = reason, tuple(frames)
        where = f"frame {self.frames[0]}: " if len(self.frames) == 1 else (f"frames {list(self.frames)}: " if self.frames else "")
        super().__init__(f"JPEG {where}{reason}")


@dataclass
class Header:
    """What the markers up to and including SOS say about a frame."""
    h: int
    w: int
    ncomp: int
    hs: int                 # luma sampling (chroma is 1 x 1); a grayscale frame is 1 x 1 whatever its SOF says
    vs: int
    restart_interval: int   # MCUs per restart segment; 0: the scan is one segment
    quant: tuple            # per component, 64 quantisation bytes in zig-zag order as the DQT segment holds them
    dc: tuple               # per component, the DHT payload of its DC table: 16 counts, then the symbols
    ac: tuple
    scan_start: int         # the offset of the first entropy-coded byte

    @property
    def mcus(self) -> tuple[int, int]:
        return -(-self.w // (8 * self.hs)), -(-self.h // (8 * self.vs))

    @property
    def blocks(self) -> int:
        mx, my = self.mcus
        return mx * my * (self.hs * self.vs + (2 if self.ncomp == 3 else 0))


_SOF_REFUSED = {0xC2: "progressive coding", 0xC3: "lossless coding", 0xC5: "hierarchical coding", 0xC6: "progressive coding (hierarchical)",
                0xC7: "lossless coding", 0xC9: "arithmetic coding", 0xCA: "arithmetic coding (progressive)", 0xCB: "arithmetic coding",
                0xCD: "arithmetic coding", 0xCE: "arithmetic coding (progressive)", 0xCF: "arithmetic coding"}


def parse_header(data: bytes) -> Header:
    """Walk the markers of one frame up to its scan.  Raises JpegError with the reason for everything outside the scope."""
    if len(data) < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise JpegError("missing SOI")
    pos, n = 2, len(data)
    quant: dict = {}
    huff: dict = {}
    sof = None
    jfif = False
    ri = 0
    while True:
        if pos + 4 > n:
            raise JpegError("missing SOS" if sof else "missing SOF")
        if data[pos] != 0xFF:
            raise JpegError(f"no marker at byte {pos}")
        while pos < n and data[pos] == 0xFF:      # fill bytes
            pos += 1
        if pos + 2 >= n:
            raise JpegError("missing SOS" if sof else "missing SOF")
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise JpegError("missing SOS" if sof else "missing SOF")
        size = (data[pos] << 8) | data[pos + 1]
        if size < 2 or pos + size > n:
            raise JpegError(f"marker FF{m:02X} runs past the end of the stream")
        body = data[pos + 2: pos + size]
        pos += size
        if m in _SOF_REFUSED:
            raise JpegError(_SOF_REFUSED[m])
        if m in (0xC0, 0xC1):
            if sof is not None:
                raise JpegError("several SOF markers")
            if len(body) < 6:
                raise JpegError("truncated SOF")
            precision, h, w, ncomp = body[0], (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            if precision != 8:
                raise JpegError(f"{precision}-bit precision")
            if h == 0 or w == 0:
                raise JpegError("dimensions of 0")
            if ncomp == 4:
                raise JpegError("4 components")
            if ncomp not in (1, 3) or len(body) < 6 + 3 * ncomp:
                raise JpegError(f"{ncomp} components")
            sof = (h, w, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(ncomp)])
        elif m == 0xC4:
            at = 0
            while at < len(body):
                if at + 17 > len(body):
                    raise JpegError("truncated DHT")
                count = sum(body[at + 1: at + 17])
                if (body[at] & 0xEF) > 3 or count > 256 or at + 17 + count > len(body):
                    raise JpegError("bad Huffman table")
                huff[body[at]] = bytes(body[at + 1: at + 17 + count])
                at += 17 + count
        elif m == 0xDB:
            at = 0
            while at < len(body):
                if body[at] >> 4:
                    raise JpegError("16-bit quantisation tables")
                if (body[at] & 15) > 3 or at + 65 > len(body):
                    raise JpegError("bad quantisation table")
                quant[body[at] & 15] = bytes(body[at + 1: at + 65])
                at += 65
        elif m == 0xDD:
            if len(body) < 2:
                raise JpegError("truncated DRI")
            ri = (body[0] << 8) | body[1]
        elif m == 0xDC:
            raise JpegError("DNL")
        elif m == 0xEE and body[:5] == b"Adobe":
            raise JpegError("Adobe APP14 segment")
        elif m == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xDA:
            if sof is None:
                raise JpegError("missing SOF")
            break
    h, w, comps = sof
    ncomp = len(comps)
    if not jfif and tuple(c[0] for c in comps) == (0x52, 0x47, 0x42):
        raise JpegError("RGB component ids without JFIF")
    if len(body) < 1 or body[0] != ncomp or len(body) < 4 + 2 * ncomp:
        raise JpegError("several scans")      # a scan of fewer components than the frame has: the others follow in scans of their own
    sel = {}
    for i in range(ncomp):
        sel[body[1 + 2 * i]] = (body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15)
    if [c[0] for c in comps] != [body[1 + 2 * i] for i in range(ncomp)]:
        raise JpegError("scan components out of the frame's order")
    if tuple(body[1 + 2 * ncomp: 4 + 2 * ncomp]) != (0, 63, 0):
        raise JpegError("progressive coding")
    if ncomp == 1:
        hs = vs = 1
    else:
        (hs, vs), chroma = comps[0][1:3], [c[1:3] for c in comps[1:]]
        if chroma != [(1, 1), (1, 1)] or (hs, vs) not in ((1, 1), (2, 1), (2, 2)):
            raise JpegError("sampling factors " + " ".join(f"{a}x{b}" for _, a, b, _ in comps))
    try:
        q = tuple(quant[c[3]] for c in comps)
        dc = tuple(huff[sel[c[0]][0]] for c in comps)
        ac = tuple(huff[0x10 | sel[c[0]][1]] for c in comps)
    except KeyError:
        raise JpegError("a table the scan names is missing") from None
    return Header(h, w, ncomp, hs, vs, ri, q, dc, ac, pos)


def huffman_table(payload: bytes) -> np.ndarray:
    """The decode table (VSJ_HUFF_BYTES bytes, the layout include/vicasplat_jpeg.h states) of a DHT payload: 16 counts, then the symbols."""
    counts, symbols = payload[:16], payload[16:]
    look = np.zeros(1 << LOOK_BITS, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    vals = np.zeros(256, np.uint8)
    vals[:len(symbols)] = np.frombuffer(symbols, np.uint8)
    code = k = 0
    for length in range(1, 17):
        cnt = counts[length - 1]
        if cnt:
            valoff[length] = k - code
            if length <= LOOK_BITS:
                for i in range(cnt):
                    shift = LOOK_BITS - length
                    look[(code + i) << shift: (code + i + 1) << shift] = (length << 8) | symbols[k + i]
            code += cnt
            k += cnt
            maxcode[length] = code - 1
        if code > 1 << length:
            raise JpegError("bad Huffman table")
        code <<= 1
    return np.concatenate([look.view(np.uint8), maxcode.view(np.uint8), valoff.view(np.uint8), vals])


@dataclass
class PackedBatch:
    """The host side of one vsj_decode call."""
    buffer: np.ndarray              # uint8: frames | segs | quant | huff | bytes, as include/vicasplat_jpeg.h lays them out
    n: int
    h: int
    w: int
    segments: int
    max_frame_segments: int
    n_quant: int
    n_huff: int
    blocks: int
    frames: np.ndarray              # views of the sections of `buffer`
    segs: np.ndarray
    quant: np.ndarray
    huff: np.ndarray
    bytes_at: int                   # where the compressed bytes start in `buffer`
    tensor: Tensor | None = None    # the (pinned) tensor that owns `buffer`, when there is one


def _as_bytes(image) -> bytes:
    if isinstance(image, (bytes, bytearray, memoryview)):
        return bytes(image)
    if isinstance(image, Tensor):
        if image.dtype != torch.uint8 or image.dim() != 1:
            raise TypeError(f"a JPEG frame is a byte string or a 1-D uint8 tensor, got {image.dtype} {tuple(image.shape)}")
        return image.cpu().numpy().tobytes()
    if isinstance(image, np.ndarray) and image.dtype == np.uint8 and image.ndim == 1:
        return image.tobytes()
    raise TypeError(f"a JPEG frame is a byte string or a 1-D uint8 tensor, got {type(image).__name__}")


def pack_jpeg_batch(images, *, pin: bool = False) -> PackedBatch:
    """Parse the frames and build the packed buffer of one call.  Host only: no GPU is touched.  All frames share (h, w)."""
    datas = [_as_bytes(im) for im in images]
    n = len(datas)
    if n == 0:
        raise ValueError("pack_jpeg_batch: no frames")
    # ---- the headers: frames of one encoder carry the same header bytes, parsed once
    headers: list[Header] = []
    last = None
    for i, d in enumerate(datas):
        try:
            if last is None or not d.startswith(last[0]):
                hd = parse_header(d)
                last = (d[:hd.scan_start], hd)
            headers.append(last[1])
        except JpegError as e:
            raise JpegError(e.reason, (i,)) from None
    h, w = headers[0].h, headers[0].w
    for i, hd in enumerate(headers):
        if (hd.h, hd.w) != (h, w):
            raise ValueError(f"pack_jpeg_batch: frame {i} is {hd.w} x {hd.h}, frame 0 is {w} x {h}: the frames of a call share one size")
    quant_ids: dict = {}
    huff_ids: dict = {}
    distinct = {id(hd): hd for hd in headers}
    words = {}
    for key, hd in distinct.items():
        mx, my = hd.mcus
        total = mx * my
        nseg = -(-total // hd.restart_interval) if hd.restart_interval else 1
        row = np.zeros(FRAME_WORDS, np.int32)
        row[[L.VSJ_F_NCOMP, L.VSJ_F_HS, L.VSJ_F_VS, L.VSJ_F_MCUS_X, L.VSJ_F_MCUS_Y, L.VSJ_F_NSEG]] = (hd.ncomp, hd.hs, hd.vs, mx, my, nseg)
        for c in range(hd.ncomp):
            row[L.VSJ_F_QUANT + c] = quant_ids.setdefault(hd.quant[c], len(quant_ids))
            row[L.VSJ_F_DC + c] = huff_ids.setdefault(hd.dc[c], len(huff_ids))
            row[L.VSJ_F_AC + c] = huff_ids.setdefault(hd.ac[c], len(huff_ids))
        words[key] = (row, nseg, hd.blocks)
    # ---- the buffer
    nsegs = np.array([words[id(hd)][1] for hd in headers], np.int64)
    nblocks = np.array([words[id(hd)][2] for hd in headers], np.int64)
    segments, blocks = int(nsegs.sum()), int(nblocks.sum())
    if blocks >= 1 << 31:
        raise ValueError(f"pack_jpeg_batch: {blocks} blocks in one call exceed 2^31 - 1")
    lengths = np.array([len(d) for d in datas], np.int64)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    nbytes = int(starts[-1])
    at_segs = n * FRAME_WORDS * 4
    at_quant = at_segs + segments * SEG_WORDS * 4
    at_huff = at_quant + len(quant_ids) * 128
    at_bytes = at_huff + len(huff_ids) * HUFF_BYTES
    size = (at_bytes + nbytes + 15) & ~15
    if nbytes >= 1 << 31:
        raise ValueError(f"pack_jpeg_batch: {nbytes} compressed bytes in one call exceed 2^31 - 1")
    # The sections are built in ordinary host memory and the markers searched in the joined streams; the (pinned) buffer of the call is
    # allocated after the last refusal, so that no refusal touches the GPU's runtime.
    head = np.zeros(at_bytes, np.uint8)
    frames = head[:at_segs].view(np.int32).reshape(n, FRAME_WORDS)
    segs = head[at_segs:at_quant].view(np.int32).reshape(segments, SEG_WORDS)
    quant = head[at_quant:at_huff].view(np.uint16).reshape(len(quant_ids), 64)
    huff = head[at_huff:at_bytes].reshape(len(huff_ids), HUFF_BYTES)
    for payload, i in quant_ids.items():
        quant[i, ZIGZAG] = np.frombuffer(payload, np.uint8)
    for payload, i in huff_ids.items():
        huff[i] = huffman_table(payload)
    data = np.frombuffer(b"".join(datas), np.uint8)
    seg0 = np.concatenate([[0], np.cumsum(nsegs)])
    block0 = np.concatenate([[0], np.cumsum(nblocks)])
    keys = list(distinct)
    frames[:] = np.stack([words[key][0] for key in keys])[[keys.index(id(hd)) for hd in headers]]
    frames[:, L.VSJ_F_SEG0] = seg0[:-1]
    frames[:, L.VSJ_F_BLOCK0] = block0[:-1]
    # ---- the markers inside the scans of all frames: one search for FF followed by neither 00 nor FF
    ff = np.flatnonzero(data[:-1] == 0xFF)
    follow = data[ff + 1]
    keep = (follow != 0) & (follow != 0xFF)
    marks, codes = ff[keep], follow[keep]
    ends = np.flatnonzero((codes & 0xF8) != 0xD0)       # indices into marks of the markers that are no RSTn
    scan = starts[:-1] + np.array([hd.scan_start for hd in headers], np.int64)
    lo = np.searchsorted(marks, scan)
    first_end = np.searchsorted(ends, lo)
    # the first marker of every scan that is no RSTn must be the frame's EOI, with the restart markers the interval asks for before it
    totals = np.array([hd.mcus[0] * hd.mcus[1] for hd in headers], np.int64)
    if len(ends):
        k = ends[np.minimum(first_end, len(ends) - 1)]
        good = (first_end < len(ends)) & (marks[k] < starts[1:]) & (codes[k] == 0xD9) & (k - lo == nsegs - 1)
    else:
        k, good = np.zeros(n, np.int64), np.zeros(n, bool)
    for i in np.flatnonzero(~good):
        stop = int(starts[i + 1])
        if first_end[i] >= len(ends) or marks[k[i]] >= stop:
            raise JpegError("missing EOI", (i,))
        if codes[k[i]] == 0xDC:
            raise JpegError("DNL", (i,))
        if codes[k[i]] != 0xD9:
            rest = codes[k[i]:np.searchsorted(marks, stop)]
            raise JpegError("several scans" if (rest == 0xDA).any() else "missing EOI", (i,))
        raise JpegError(f"{k[i] - lo[i]} restart markers where the restart interval asks for {nsegs[i] - 1}", (i,))
    single = np.flatnonzero(nsegs == 1)          # the scans without restart markers, all at once
    s = segs[seg0[single]]
    s[:, 0], s[:, 1], s[:, 2], s[:, 3] = scan[single], marks[k[single]], 0, totals[single]
    for j in np.flatnonzero(data[np.maximum(s[:, 1] - 1, 0)] == 0xFF):      # fill bytes before the marker
        while s[j, 1] > s[j, 0] and data[s[j, 1] - 1] == 0xFF:
            s[j, 1] -= 1
    segs[seg0[single]] = s
    for i in np.flatnonzero(nsegs > 1):
        rst = marks[lo[i]:k[i]]
        begin = np.concatenate([[scan[i]], rst + 2])
        end = np.concatenate([rst, [marks[k[i]]]])
        for j in np.flatnonzero(data[np.maximum(end - 1, 0)] == 0xFF):      # fill bytes before a marker
            while end[j] > begin[j] and data[end[j] - 1] == 0xFF:
                end[j] -= 1
        per = headers[i].restart_interval
        first = np.arange(nsegs[i], dtype=np.int64) * per
        s = segs[seg0[i]:seg0[i + 1]]
        s[:, 0], s[:, 1], s[:, 2], s[:, 3] = begin, end, first, np.minimum(per, totals[i] - first)
    tensor = torch.empty(size, dtype=torch.uint8, pin_memory=True) if pin and torch.cuda.is_available() else None
    buf = tensor.numpy() if tensor is not None else np.empty(size, np.uint8)
    buf[:at_bytes] = head
    buf[at_bytes:at_bytes + nbytes] = data      # the compressed bytes, in one piece
    buf[at_bytes + nbytes:] = 0
    frames = buf[:at_segs].view(np.int32).reshape(n, FRAME_WORDS)
    segs = buf[at_segs:at_quant].view(np.int32).reshape(segments, SEG_WORDS)
    quant = buf[at_quant:at_huff].view(np.uint16).reshape(len(quant_ids), 64)
    huff = buf[at_huff:at_bytes].reshape(len(huff_ids), HUFF_BYTES)
    return PackedBatch(buf, n, h, w, segments, int(nsegs.max()), len(quant_ids), len(huff_ids), blocks, frames, segs, quant, huff, at_bytes, tensor)


def decode_packed(packed: PackedBatch, device: torch.device, buffer: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """Run vsj_decode on a packed batch: (uint8 [N, h, w, 3], int32 status [N]) on the device; no synchronisation.  `buffer`: the packed
    bytes already on the device (a graph replay keeps them there)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("vicasplat_amd kernels need a HIP device; there is no CPU fallback")
    if buffer is None:
        src = packed.tensor if packed.tensor is not None else torch.from_numpy(packed.buffer)
        buffer = src.to(device, non_blocking=True)
    need = L.call("vsj_workspace_bytes", device, packed.blocks, packed.segments)
    workspace = torch.empty(need, dtype=torch.uint8, device=device)
    out = torch.empty(packed.n, packed.h, packed.w, 3, dtype=torch.uint8, device=device)
    status = torch.empty(packed.n, dtype=torch.int32, device=device)
    L.call("vsj_decode", device, L.ptr(buffer), buffer.numel(), packed.n, packed.h, packed.w, packed.segments, packed.max_frame_segments,
           packed.n_quant, packed.n_huff, packed.blocks, L.ptr(workspace), need, L.ptr(out), L.ptr(status))
    return out, status


def status_names(word: int) -> str:
    return "|".join(name for name, bit in STATUS_BITS.items() if word & bit) or "clean"


def decode_jpeg_batch(images, *, device=None, check: bool = True, return_status: bool = False):
    """JPEG frames -> uint8 [N, h, w, 3] on the device, the bytes PIL's Image.open(...).convert("RGB") gives.

    images: byte strings or 1-D uint8 tensors, the form example["images"][i] has in the reference's chunks; all frames of a call share
    (h, w), while sampling, tables and restart interval may differ per frame.
    check=True reads the per-frame status back (one synchronisation) and raises JpegError naming the frames whose entropy-coded data is
    damaged; check=False does not synchronise.  return_status=True returns (pixels, int32 status [N], 0 = clean).
    `.permute(0, 3, 1, 2)` of the result is the packed HWC view apply_crop_shim_to_views and preprocess_batch take without a copy."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("vicasplat_amd kernels need a HIP device; there is no CPU fallback")
    out, status = decode_packed(pack_jpeg_batch(images, pin=True), device)
    if check:
        words = status.cpu().numpy()
        bad = np.flatnonzero(words)
        if len(bad):
            raise JpegError("damaged entropy-coded data (" + ", ".join(f"{i}: {status_names(int(words[i]))}" for i in bad) + ")", bad.tolist())
    return (out, status) if return_status else out


def convert_images(images, device=None) -> Tensor:
    """The reference's DatasetRE10k.convert_images: float32 [N, 3, h, w] in [0, 1] -- the decode, then an exact division by 255."""
    frames = decode_jpeg_batch(images, device=device)
    return rescale(frames.permute(0, 3, 1, 2), tuple(frames.shape[1:3]))      # both passes skipped: the kernel's float32(u) / 255
