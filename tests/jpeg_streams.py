"""A baseline-JPEG stream writer for the decoder's conformance tests (tests/test_jpeg_streams.py on the
host checker, tests/test_gpu_jpeg_streams.py on the device).  PIL's encoder only ever writes one
interleaved scan with two quantisation tables defined once; csrc/jpeg.hip claims several scans, restart
intervals, 16-bit tables and SOF1, and its kernels have edges (one block, cw == 1, ch == 1, blocks with
no coefficient) no PIL-written file of a smooth picture reaches.  This writer produces those files from
real pixels, so that PIL's libjpeg-turbo stays a defined oracle for them:

    planes  -> float forward DCT -> round-to-nearest quantisation -> Huffman coding (the standard
    tables, parsed at import from a file PIL writes without `optimize`: no table is typed in here)

with the scan structure, restart interval, table precision, frame marker, fill bytes, Huffman table ids,
component ids, JFIF segment and the place of every DQT chosen by the caller.  Pure numpy + struct.

Geometry (T.81 A.1.1, A.2): component c of an H x W image with sampling (h, v) is cw x ch =
ceil(W h / hmax) x ceil(H v / vmax) samples; an interleaved scan codes h x v blocks of it per MCU over
ceil(W / 8 hmax) x ceil(H / 8 vmax) MCUs (its block grid padded to that), a non-interleaved scan one
block per MCU over the component's own ceil(cw / 8) x ceil(ch / 8) grid.
"""
import functools
import io
import struct

import numpy as np
from PIL import Image

# zig-zag position -> natural (row-major) index: diagonals r + c, odd ones walked down, even ones up
ZIGZAG = np.array(sorted(range(64), key=lambda i: (i // 8 + i % 8, i // 8 if (i // 8 + i % 8) % 2 else i % 8)))

SAMPLINGS = {"gray": [(1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)]}


def segments(data):
    """(marker, payload offset, payload length) of every marker segment up to the first SOS."""
    pos, out = 2, []
    while pos + 4 <= len(data):
        assert data[pos] == 0xFF
        m = data[pos + 1]
        n = struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((m, pos + 4, n - 2))
        if m == 0xDA:
            break
        pos += 2 + n
    return out


def _standard_huffman():
    """{(class, id): {symbol: (code, length)}} of the four tables PIL writes when it does not optimise
    (T.81 K.3-K.6): class 0 = DC, 1 = AC; id 0 = luminance, 1 = chrominance; and their DHT payloads."""
    b = io.BytesIO()
    Image.new("RGB", (8, 8)).save(b, "JPEG")
    data = b.getvalue()
    codes, raw = {}, {}
    for m, at, n in segments(data):
        if m != 0xC4:
            continue
        p = at
        while p < at + n:
            tc, th = data[p] >> 4, data[p] & 15
            bits = list(data[p + 1:p + 17])
            vals = data[p + 17:p + 17 + sum(bits)]
            raw[tc, th] = bytes(data[p + 1:p + 17 + sum(bits)])
            table, code, k = {}, 0, 0
            for length, cnt in enumerate(bits, 1):
                for _ in range(cnt):
                    table[vals[k]] = (code, length)
                    code += 1
                    k += 1
                code <<= 1
            codes[tc, th] = table
            p += 17 + sum(bits)
    assert sorted(codes) == [(0, 0), (0, 1), (1, 0), (1, 1)], sorted(codes)
    return codes, raw


HUFF, HUFF_RAW = _standard_huffman()


class Geometry:
    def __init__(self, H, W, samp):
        self.H, self.W, self.samp = H, W, list(samp)
        self.hmax = max(h for h, _ in samp)
        self.vmax = max(v for _, v in samp)
        self.mcus_x = -(-W // (8 * self.hmax))
        self.mcus_y = -(-H // (8 * self.vmax))
        self.cw = [-(-W * h // self.hmax) for h, _ in samp]
        self.ch = [-(-H * v // self.vmax) for _, v in samp]
        self.bw = [self.mcus_x * h for h, _ in samp]
        self.bh = [self.mcus_y * v for _, v in samp]


# ------------------------------------------------------------------------------------------ content
def field(h, w, seed, noise):
    """A seeded smooth field plus noise as uint8 [h, w]: noise 0 none (DC-only blocks under a coarse
    quantiser), 1 moderate (sigma 14: under a flat quantiser of 48 about one coefficient in ten
    survives, so zero runs pass 16), 2 heavy (every coefficient under a fine quantiser)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a, b, c, d = rs.uniform(-1, 1, 4)
    f = 128 + 60 * a * np.sin(0.21 * x + 3 * b) + 50 * c * np.cos(0.17 * y + 3 * d) + 1.5 * (a * x + c * y)
    f = f + (0.0, 14.0, 110.0)[noise] * rs.standard_normal((h, w))
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def make_planes(geo, seed, noise):
    """Component planes at component resolution, edge-replicated to the MCU-padded block grid."""
    out = []
    for c in range(len(geo.samp)):
        p = field(geo.ch[c], geo.cw[c], seed * 7 + c, noise)
        out.append(np.pad(p, ((0, geo.bh[c] * 8 - geo.ch[c]), (0, geo.bw[c] * 8 - geo.cw[c])), mode="edge"))
    return out


def flat(q):
    return np.full(64, q, np.int64)


def ramp(base, step):
    """A quantisation table growing with frequency (natural order)."""
    u, v = np.mgrid[0:8, 0:8]
    return (base + step * (u + v)).reshape(64).astype(np.int64)


_k = np.arange(8)
_DCT = 0.5 * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)
_DCT[0] /= np.sqrt(2.0)


def quantise(planes, quants):
    """Per component: int coefficients [bh, bw, 64] in zig-zag order, of the float forward DCT of the
    level-shifted plane divided by the component's quantiser (natural order) and rounded to nearest."""
    out = []
    for p, q in zip(planes, quants):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = (p.astype(np.float64) - 128).reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        co = np.einsum("ux,abxy,vy->abuv", _DCT, blocks, _DCT).reshape(bh, bw, 64)
        z = np.rint(co / np.asarray(q, np.float64)).astype(np.int64)[:, :, ZIGZAG]
        # what an encoder can produce from 8-bit pixels, and what baseline Huffman tables can code
        assert np.abs(z[:, :, 0]).max() <= 1024 and np.abs(z[:, :, 1:]).max(initial=0) <= 1023
        out.append(z)
    return out


def block_kinds(coefs):
    """How many blocks are DC-only, hold a zero run of 16 or more before a coefficient (ZRL), and
    have a nonzero last coefficient (no EOB)."""
    n = dict(dc_only=0, zrl=0, full=0)
    for z in coefs:
        for blk in z.reshape(-1, 64):
            nz = np.flatnonzero(blk[1:]) + 1
            n["dc_only"] += nz.size == 0
            n["zrl"] += bool(nz.size and np.diff(np.concatenate([[0], nz])).max() > 16)
            n["full"] += blk[63] != 0
    return n


# ------------------------------------------------------------------------------------------ entropy coding
class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, length):
        self.acc = (self.acc << length) | value
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):  # pad the last byte with one bits (T.81 F.1.2.3)
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    s = abs(v).bit_length()
    return s, (v if v > 0 else v + (1 << s) - 1)


def _code_block(bits, z, pred, dc, ac):
    s, extra = _magnitude(int(z[0]) - pred)
    bits.put(*dc[s])
    if s:
        bits.put(extra, s)
    run = 0
    for k in range(1, 64):
        v = int(z[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])
            run -= 16
        s, extra = _magnitude(v)
        bits.put(*ac[(run << 4) | s])
        bits.put(extra, s)
        run = 0
    if run:
        bits.put(*ac[0x00])
    return int(z[0])


def _scan_blocks(geo, comps):
    """Per MCU of a scan over `comps`: its (slot in the scan, component, block row, block column)."""
    if len(comps) == 1:
        c = comps[0]
        nx, ny = -(-geo.cw[c] // 8), -(-geo.ch[c] // 8)
        return [[(0, c, my, mx)] for my in range(ny) for mx in range(nx)]
    mcus = []
    for my in range(geo.mcus_y):
        for mx in range(geo.mcus_x):
            m = []
            for i, c in enumerate(comps):
                h, v = geo.samp[c]
                m += [(i, c, my * v + by, mx * h + bx) for by in range(v) for bx in range(h)]
            mcus.append(m)
    return mcus


def _entropy(geo, coefs, comps, restart, huff_of, fill):
    """The entropy-coded segment of one scan, RSTn markers included; and where each marker starts."""
    bits, pred, rst_at, nrst = _Bits(), [0] * len(comps), [], 0
    for n, mcu in enumerate(_scan_blocks(geo, comps)):
        if restart and n and n % restart == 0:
            bits.flush()
            rst_at.append(len(bits.out) + fill)
            bits.out += b"\xff" * fill + bytes([0xFF, 0xD0 + nrst % 8])
            nrst += 1
            pred = [0] * len(comps)
        for i, c, by, bx in mcu:
            dc, ac = huff_of(c)
            pred[i] = _code_block(bits, coefs[c][by, bx], pred[i], dc, ac)
    bits.flush()
    return bytes(bits.out), rst_at


# ------------------------------------------------------------------------------------------ the file
def write(geo, coefs, scans, tables, tq, *, ids=None, restart=0, dqt16=False, sof=0xC0, fill=0, huff_ids=(0, 1),
          jfif=True, dqt_before=None, info=None):
    """One JPEG file.
    coefs       quantise()'s output;
    scans       a list of scans, each the list of its component indices, coded in that order;
    tables      {table id: 64 values, natural order} of the DQT in the header;
    tq          each component's table id in the frame header;
    ids         component ids (default 1, 2, 3);
    restart     restart interval in MCUs of each scan (0 = none; a DRI segment otherwise);
    dqt16       16-bit DQT entries (Pq = 1);
    sof         0xC0 baseline or 0xC1 extended sequential;
    fill        0xFF fill bytes before every marker but SOI;
    huff_ids    Huffman table ids of (luminance, chrominance): the standard tables under those ids;
    jfif        write the JFIF APP0 segment;
    dqt_before  {scan index: {table id: values}}: a DQT segment just before that scan's SOS;
    info        a dict that receives 'rst': the file offset of every RSTn marker's 0xFF 0xDn.
    """
    ids = list(ids if ids is not None else range(1, len(geo.samp) + 1))
    out = bytearray(b"\xff\xd8")

    def seg(m, payload):
        out.extend(b"\xff" * fill + bytes([0xFF, m]) + struct.pack(">H", len(payload) + 2) + payload)

    def dqt(tabs):
        body = b""
        for t, vals in sorted(tabs.items()):
            z = np.asarray(vals, np.int64)[ZIGZAG]
            assert z.min() >= 1 and z.max() <= (65535 if dqt16 else 255)
            body += bytes([(16 if dqt16 else 0) | t]) + (struct.pack(">64H", *z) if dqt16 else bytes(int(x) for x in z))
        seg(0xDB, body)

    if jfif:
        seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if tables:
        dqt(tables)
    frame = struct.pack(">BHHB", 8, geo.H, geo.W, len(geo.samp))
    for c, (h, v) in enumerate(geo.samp):
        frame += bytes([ids[c], (h << 4) | v, tq[c]])
    seg(sof, frame)
    seg(0xC4, b"".join(bytes([(tc << 4) | huff_ids[k]]) + HUFF_RAW[tc, k] for k in (0, 1) for tc in (0, 1)))
    if restart:
        seg(0xDD, struct.pack(">H", restart))
    rst = []
    for n, comps in enumerate(scans):
        if dqt_before and n in dqt_before:
            dqt(dqt_before[n])
        head = bytes([len(comps)])
        for c in comps:
            head += bytes([ids[c], huff_ids[c > 0] * 17])
        seg(0xDA, head + b"\x00\x3f\x00")
        data, at = _entropy(geo, coefs, comps, restart, lambda c: (HUFF[0, c > 0], HUFF[1, c > 0]), fill)
        rst += [len(out) + a for a in at]
        out.extend(data)
    out.extend(b"\xff" * fill + b"\xff\xd9")
    if info is not None:
        info["rst"] = rst
    return bytes(out)


# ------------------------------------------------------------------------------------------ the cases
MID = (ramp(3, 2), ramp(5, 3))  # a moderate luminance / chrominance pair


def scan_list(kind, ncomp):
    """'il' one interleaved scan, 'ni' one scan per component, 'mixed' chrominance interleaved then
    luminance, 'yonly' the chrominance never scanned."""
    if ncomp == 1:
        return [[0]]
    return {"il": [[0, 1, 2]], "ni": [[0], [1], [2]], "mixed": [[1, 2], [0]], "yonly": [[0]]}[kind]


def stream(H, W, sampling, scans="il", q="mid", noise=1, seed=0, **opts):
    """One file of the named sampling: q 'mid' = the MID pair, a number = flat tables of that value
    (16-bit DQT and SOF1 above 255).  Returns the bytes."""
    geo = Geometry(H, W, SAMPLINGS[sampling])
    n = len(geo.samp)
    pair = MID if q == "mid" else (flat(q), flat(q))
    if q != "mid" and q > 255:
        opts.setdefault("dqt16", True)
        opts.setdefault("sof", 0xC1)
    tq = [0, 1, 1][:n]
    coefs = quantise(make_planes(geo, seed, noise), [pair[t] for t in tq])
    tables = {0: pair[0], 1: pair[1]} if n == 3 else {0: pair[0]}
    return write(geo, coefs, scan_list(scans, n) if isinstance(scans, str) else scans, tables, tq, **opts)


def redefined_table_pair(H, W, sampling="420", seed=0, noise=1, **opts):
    """Two files of the same coefficients: one defines table 0 = A, scans Y, redefines table 0 = B and
    scans Cb, Cr, every component naming table 0; its twin defines A and B once as tables 0 and 1.
    A decoder that latches a component's table at its first scan (libjpeg) decodes both alike."""
    geo = Geometry(H, W, SAMPLINGS[sampling])
    A, B = MID
    coefs = quantise(make_planes(geo, seed, noise), [A, B, B])
    ni = [[0], [1], [2]]
    return (write(geo, coefs, ni, {0: A}, [0, 0, 0], dqt_before={1: {0: B}}, **opts),
            write(geo, coefs, ni, {0: A, 1: B}, [0, 1, 1], **opts))


# (name, sampling, scans, restart, q, noise, further write() options): together gray / 4:4:4 / 4:2:2 / 4:2:0;
# interleaved, per-component and mixed scans; restart 0, 1 and 5; chrominance never scanned; q = 1, 255,
# 16-bit 300 and 2000 under SOF1; noise 0, moderate and heavy; fill bytes, Huffman ids 2 and 3, component
# ids 0 1 2, no JFIF
VARIANTS = [
    ("gray-mid", "gray", "il", 0, "mid", 1, {}),
    ("gray-q1-r1", "gray", "il", 1, 1, 2, {}),
    ("gray-q255-r5", "gray", "il", 5, 255, 0, {}),
    ("gray-q2000", "gray", "il", 0, 2000, 2, dict(fill=1)),
    ("444-il-q1", "444", "il", 0, 1, 2, {}),
    ("444-ni-q48-r1", "444", "ni", 1, 48, 1, {}),
    ("444-mixed-q255-r5", "444", "mixed", 5, 255, 2, {}),
    ("444-yonly", "444", "yonly", 0, "mid", 0, {}),
    ("444-ni-ids012-h23", "444", "ni", 0, "mid", 2, dict(ids=[0, 1, 2], huff_ids=(2, 3), sof=0xC1)),
    ("422-il-r5", "422", "il", 5, "mid", 2, {}),
    ("422-ni-q1", "422", "ni", 0, 1, 0, {}),
    ("422-mixed-q300-r1", "422", "mixed", 1, 300, 2, {}),
    ("422-yonly-q1-r5", "422", "yonly", 5, 1, 2, {}),
    ("422-il-fill-nojfif", "422", "il", 0, "mid", 1, dict(fill=1, jfif=False)),
    ("420-il-r1", "420", "il", 1, "mid", 1, {}),
    ("420-il-q1", "420", "il", 0, 1, 2, {}),
    ("420-ni-q255-r5", "420", "ni", 5, 255, 2, {}),
    ("420-mixed", "420", "mixed", 0, "mid", 0, {}),
    ("420-mixed-q2000-r1", "420", "mixed", 1, 2000, 2, {}),
    ("420-ni-q300-all", "420", "ni", 0, 300, 1, dict(ids=[0, 1, 2], huff_ids=(2, 3), jfif=False, fill=2)),
    ("420-yonly-q48-r1", "420", "yonly", 1, 48, 1, {}),
    ("420-il-q255-noise0", "420", "il", 5, 255, 0, {}),
]

# the device table: a single block, one row, one column, ch == 1, the cw <= 2 rule and the first width
# above it, one whole block, ragged on both axes, exactly one 4:2:0 MCU, just above an MCU boundary, a
# few workgroups
DEVICE_SIZES = [(1, 1), (1, 17), (17, 1), (2, 2), (9, 3), (9, 4), (9, 5), (8, 8), (9, 17), (16, 16), (17, 33), (37, 29)]
# the host list adds the other narrow widths and heights, and sizes around the block and MCU edges
HOST_SIZES = DEVICE_SIZES + [(1, 2), (2, 1), (3, 3), (4, 4), (3, 2), (17, 4), (5, 6), (4, 37), (7, 9), (15, 16),
                             (16, 17), (24, 40), (33, 8), (31, 32)]


@functools.lru_cache(maxsize=None)
def variants(H, W):
    """[(name, file bytes)] of one size: VARIANTS and the redefined-table file.  Cached: the host and
    the device tests of one run share the files."""
    out = []
    for k, (name, sampling, scans, restart, q, noise, opts) in enumerate(VARIANTS):
        out.append((name, stream(H, W, sampling, scans, q, noise, seed=H * 131 + W * 17 + k, restart=restart, **opts)))
    out.append(("420-dqt-redefined", redefined_table_pair(H, W, "420", seed=H + W, noise=2)[0]))
    out.append(("422-dqt-redefined-r5", redefined_table_pair(H, W, "422", seed=H + W + 1, noise=1, restart=5)[0]))
    return out


def pil_rgb(data):
    """PIL's decode as uint8 [3, H, W]; any warning-turned-error or exception propagates."""
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB")).transpose(2, 0, 1).copy()


@functools.lru_cache(maxsize=None)
def references(H, W):
    """PIL's pixels of variants(H, W), computed once and handed out read-only."""
    refs = []
    for _, data in variants(H, W):
        r = pil_rgb(data)
        r.setflags(write=False)
        refs.append(r)
    return refs
